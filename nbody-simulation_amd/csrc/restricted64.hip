// libnbody_hip — restricted ensembles in f64: the C entry points of nbody_restricted64_* (include/nbody_ensemble.h) over the
// driver of restricted_driver.h in the precision of ensemble_f64.h, with the tracers' launch of restricted64_kernels.h.
#include "ensemble_f64.h"
#include "restricted_driver.h"
#include "restricted64_kernels.h"

using namespace nbody;

struct Rst64 : EnsF64 {
  using Tracers = Restricted64Args;
  static constexpr const char* kCreate = "nbody_restricted64_create";
  static constexpr const char* kWho = "restricted";
  static hipError_t launch_tracers(hipStream_t s, int64_t n_worlds, const Ensemble64Args& a, Restricted64Args t) {
    return launch_restricted64_tracers(s, n_worlds, a, t);
  }
};
struct nbody_restricted64 : RestrictedState<Rst64> {};

NB_API int nbody_restricted64_create(nbody_restricted64** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_restricted64_destroy(nbody_restricted64* e) { ens_destroy(e); }
NB_API const char* nbody_restricted64_last_error(const nbody_restricted64* e) { return ens_last_error<Rst64>(e); }
NB_API int nbody_restricted64_set_params(nbody_restricted64* e, const nbody_params* p) { return ens_set_params<Rst64>(e, p); }
NB_API int nbody_restricted64_get_params(const nbody_restricted64* e, nbody_params* out) { return ens_get_params<Rst64>(e, out); }
NB_API int nbody_restricted64_upload(nbody_restricted64* e, int64_t n_worlds, int64_t n_bodies, const double* pos, const double* vel,
                                     const uint32_t* weight) {
  return rst_upload<Rst64>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_restricted64_download(nbody_restricted64* e, double* pos, double* vel) { return ens_download<Rst64>(e, pos, vel); }
NB_API int64_t nbody_restricted64_num_worlds(const nbody_restricted64* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_restricted64_num_bodies(const nbody_restricted64* e) { return e ? e->n_bodies : 0; }
NB_API int64_t nbody_restricted64_num_tracers(const nbody_restricted64* e) { return rst_num_tracers<Rst64>(e); }
NB_API int nbody_restricted64_tracers_upload(nbody_restricted64* e, int64_t n_worlds, int64_t n_tracers, const double* pos, const double* vel) {
  return rst_tracers_upload<Rst64>(e, n_worlds, n_tracers, pos, vel);
}
NB_API int nbody_restricted64_tracers_download(nbody_restricted64* e, double* pos, double* vel) { return rst_tracers_download<Rst64>(e, pos, vel); }
NB_API int nbody_restricted64_update(nbody_restricted64* e, double delta, int n_steps, nbody_counting* counter) {
  return rst_update<Rst64>(e, delta, n_steps, counter);
}
NB_API int nbody_restricted64_accel(nbody_restricted64* e, double* acc_xy) { return rst_accel<Rst64>(e, acc_xy); }
NB_API int nbody_restricted64_tracers_accel(nbody_restricted64* e, double* acc_xy) { return rst_tracers_accel<Rst64>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_restricted64(nbody_restricted64* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out) {
  return ens_frames<Rst64>(e, height, render_px, rgba_out, rst_rows<Rst64>(e), with_tracers != 0);
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_restricted64(nbody_restricted64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out,
                                     uint64_t* offsets_out, uint64_t* step_out) {
  return ens_deltas<Rst64>(e, flags, out, cap, bytes_out, offsets_out, step_out, rst_rows<Rst64>(e));
}
// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_sweep_restricted64(nbody_restricted64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                                    nbody_counting* counter) {
  return rst_sweep<Rst64>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_restricted64(nbody_restricted64* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<Rst64>(e, flags, height, ref, out, rst_rows<Rst64>(e));
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_restricted64(nbody_restricted64* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, double* nn_d2,
                                         uint32_t* close) {
  return ens_encounters<Rst64>(e, flags, limit2, out, nn_index, nn_d2, close, rst_rows<Rst64>(e));
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_restricted64(nbody_restricted64* e, uint32_t flags, double delta, int n_steps, int stride, const float* limit2, uint32_t height,
                                    nbody_world_watch* out, const nbody_watch_rows_f64* rows, nbody_counting* counter) {
  return ens_watch_with<Rst64>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, rst_rows<Rst64>(e),
                               [e](const Rst64::Args& a) { return rst_launch_step<Rst64>(e, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_restricted64(nbody_restricted64* e, uint32_t flags, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f64* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<Rst64>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, rst_rows<Rst64>(e),
        [e](const Rst64::Args& a) { return rst_launch_step<Rst64>(e, a); });
}
