// libnbody_hip — ensembles: the C entry points of nbody_ensemble_* (include/nbody_hip.h) over the driver of ensemble_driver.h,
// and what is f32 about them: the masses uploaded as `weight as f32`, the arith rule of the f32 direct step, the kernel of
// ensemble_kernels.hip.
#include "ensemble_driver.h"

using namespace nbody;

struct EnsF32 {
  using Real = float;
  using Vec2 = float2;
  using Mass = float;
  using Args = EnsembleArgs;
  static constexpr const char* kCreate = "nbody_ensemble_create";
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
  static hipError_t launch(hipStream_t s, int64_t n_worlds, const EnsembleArgs& a) { return launch_ensemble_step(s, n_worlds, a); }
};
struct nbody_ensemble : EnsembleState<EnsF32> {};

NB_API int nbody_ensemble_create(nbody_ensemble** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_ensemble_destroy(nbody_ensemble* e) { ens_destroy(e); }
NB_API const char* nbody_ensemble_last_error(const nbody_ensemble* e) { return ens_last_error<EnsF32>(e); }
NB_API int nbody_ensemble_set_params(nbody_ensemble* e, const nbody_params* p) { return ens_set_params<EnsF32>(e, p); }
NB_API int nbody_ensemble_get_params(const nbody_ensemble* e, nbody_params* out) { return ens_get_params<EnsF32>(e, out); }
NB_API int nbody_ensemble_upload_f32(nbody_ensemble* e, int64_t n_worlds, int64_t n_bodies, const float* pos, const float* vel,
                                     const uint32_t* weight) {
  return ens_upload<EnsF32>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_ensemble_download_f32(nbody_ensemble* e, float* pos, float* vel) { return ens_download<EnsF32>(e, pos, vel); }
NB_API int64_t nbody_ensemble_num_worlds(const nbody_ensemble* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_ensemble_num_bodies(const nbody_ensemble* e) { return e ? e->n_bodies : 0; }
NB_API int nbody_ensemble_update_f32(nbody_ensemble* e, float delta, int n_steps, nbody_counting* counter) {
  return ens_update<EnsF32>(e, delta, n_steps, counter);
}
NB_API int nbody_ensemble_accel_f32(nbody_ensemble* e, float* acc_xy) { return ens_accel<EnsF32>(e, acc_xy); }
