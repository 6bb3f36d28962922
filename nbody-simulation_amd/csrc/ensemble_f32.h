// What is f32 about an ensemble, for the driver of ensemble_driver.h: the masses uploaded as `weight as f32`, the arith rule of the
// f32 direct step, the kernel of ensemble_kernels.hip.  Internal; ensemble.hip (nbody_ensemble_*), ragged.hip (nbody_ragged_*),
// restricted.hip (nbody_restricted_*, which adds the tracers' launch for restricted_driver.h) and rr.hip (nbody_rr_*, which adds
// both the ragged launch and the tracers' launch over work items for rr_driver.h) build their handles over it.
#pragma once
#include "ensemble_driver.h"

namespace nbody {

struct EnsF32 {
  using Real = float;
  using Vec2 = float2;
  using Mass = float;
  using Args = EnsembleArgs;
  static constexpr const char* kCreate = "nbody_ensemble_create";
  static constexpr const char* kWho = "ensemble";
  static const float* stage(const uint32_t* weight, size_t rows, std::vector<float>& tmp) {
    tmp.resize(rows);
    for (size_t i = 0; i < rows; ++i) tmp[i] = weight ? (float)weight[i] : 1.0f;  // `weight as f32`, main.rs:360
    return tmp.data();
  }
  static void route(EnsembleArgs& a, const float* mass, const nbody_params& p) {
    a.mass = mass;
    a.clamp = p.clamp;
    a.arith = direct_arith_f32(p.arith, p.clamp);  // a clamp below kFastClampFloor (or NaN): every world EXACT
  }
  using SweepWorld = EnsSweepWorld;
  static EnsSweepWorld sweep_world(float delta, float clamp, int32_t steps) { return EnsSweepWorld{delta, clamp, steps, 0}; }
  static void sweep_route(EnsembleArgs& a, const nbody_params& p) { a.arith = p.arith; }  // (direct_arith_f32's clamp test: per world, in the kernel)
  static hipError_t launch(hipStream_t s, int64_t n_worlds, const EnsembleArgs& a) { return launch_ensemble_step(s, n_worlds, a); }
  static hipError_t launch_resident(hipStream_t s, int64_t n_worlds, const uint2* worlds, size_t lds_bytes, const EnsembleArgs& a) {
    return launch_ensemble_resident(s, n_worlds, worlds, lds_bytes, a);
  }
  static size_t resident_lds_bytes(int n_bodies) { return ensemble_resident_lds_bytes(n_bodies); }
};

}  // namespace nbody
