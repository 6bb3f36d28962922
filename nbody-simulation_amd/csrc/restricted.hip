// libnbody_hip — restricted ensembles: the C entry points of nbody_restricted_* (include/nbody_ensemble.h) over the driver of
// restricted_driver.h in the precision of ensemble_f32.h, with the tracers' launch of restricted_kernels.h.
#include "ensemble_f32.h"
#include "restricted_driver.h"
#include "restricted_kernels.h"

using namespace nbody;

struct RstF32 : EnsF32 {
  using Tracers = RestrictedArgs;
  static constexpr const char* kCreate = "nbody_restricted_create";
  static constexpr const char* kWho = "restricted";
  static hipError_t launch_tracers(hipStream_t s, int64_t n_worlds, const EnsembleArgs& a, RestrictedArgs t) {
    return launch_restricted_tracers(s, n_worlds, a, t);
  }
};
struct nbody_restricted : RestrictedState<RstF32> {};

NB_API int nbody_restricted_create(nbody_restricted** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_restricted_destroy(nbody_restricted* e) { ens_destroy(e); }
NB_API const char* nbody_restricted_last_error(const nbody_restricted* e) { return ens_last_error<RstF32>(e); }
NB_API int nbody_restricted_set_params(nbody_restricted* e, const nbody_params* p) { return ens_set_params<RstF32>(e, p); }
NB_API int nbody_restricted_get_params(const nbody_restricted* e, nbody_params* out) { return ens_get_params<RstF32>(e, out); }
NB_API int nbody_restricted_upload_f32(nbody_restricted* e, int64_t n_worlds, int64_t n_bodies, const float* pos, const float* vel,
                                       const uint32_t* weight) {
  return rst_upload<RstF32>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_restricted_download_f32(nbody_restricted* e, float* pos, float* vel) { return ens_download<RstF32>(e, pos, vel); }
NB_API int64_t nbody_restricted_num_worlds(const nbody_restricted* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_restricted_num_bodies(const nbody_restricted* e) { return e ? e->n_bodies : 0; }
NB_API int64_t nbody_restricted_num_tracers(const nbody_restricted* e) { return rst_num_tracers<RstF32>(e); }
NB_API int nbody_restricted_tracers_upload_f32(nbody_restricted* e, int64_t n_worlds, int64_t n_tracers, const float* pos, const float* vel) {
  return rst_tracers_upload<RstF32>(e, n_worlds, n_tracers, pos, vel);
}
NB_API int nbody_restricted_tracers_download_f32(nbody_restricted* e, float* pos, float* vel) { return rst_tracers_download<RstF32>(e, pos, vel); }
NB_API int nbody_restricted_update_f32(nbody_restricted* e, float delta, int n_steps, nbody_counting* counter) {
  return rst_update<RstF32>(e, delta, n_steps, counter);
}
NB_API int nbody_restricted_accel_f32(nbody_restricted* e, float* acc_xy) { return rst_accel<RstF32>(e, acc_xy); }
NB_API int nbody_restricted_tracers_accel_f32(nbody_restricted* e, float* acc_xy) { return rst_tracers_accel<RstF32>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_restricted(nbody_restricted* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out) {
  return ens_frames<RstF32>(e, height, render_px, rgba_out, rst_rows<RstF32>(e), with_tracers != 0);
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_restricted(nbody_restricted* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                                   uint64_t* step_out) {
  return ens_deltas<RstF32>(e, flags, out, cap, bytes_out, offsets_out, step_out, rst_rows<RstF32>(e));
}
// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_sweep_restricted(nbody_restricted* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                                  nbody_counting* counter) {
  return rst_sweep<RstF32>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_restricted(nbody_restricted* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<RstF32>(e, flags, height, ref, out, rst_rows<RstF32>(e));
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_restricted(nbody_restricted* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, float* nn_d2,
                                       uint32_t* close) {
  return ens_encounters<RstF32>(e, flags, limit2, out, nn_index, nn_d2, close, rst_rows<RstF32>(e));
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_restricted(nbody_restricted* e, uint32_t flags, float delta, int n_steps, int stride, const float* limit2, uint32_t height,
                                  nbody_world_watch* out, const nbody_watch_rows_f32* rows, nbody_counting* counter) {
  return ens_watch_with<RstF32>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, rst_rows<RstF32>(e),
                                [e](const RstF32::Args& a) { return rst_launch_step<RstF32>(e, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_restricted(nbody_restricted* e, uint32_t flags, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f32* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<RstF32>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, rst_rows<RstF32>(e),
        [e](const RstF32::Args& a) { return rst_launch_step<RstF32>(e, a); });
}
