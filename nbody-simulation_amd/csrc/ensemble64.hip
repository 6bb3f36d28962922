// libnbody_hip — ensembles in f64: the C entry points of nbody_ensemble64_* (include/nbody_ensemble.h) over the driver of
// ensemble_driver.h in the precision of ensemble_f64.h.
#include "ensemble_f64.h"

using namespace nbody;

struct nbody_ensemble64 : EnsembleState<EnsF64> {};

NB_API int nbody_ensemble64_create(nbody_ensemble64** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_ensemble64_destroy(nbody_ensemble64* e) { ens_destroy(e); }
NB_API const char* nbody_ensemble64_last_error(const nbody_ensemble64* e) { return ens_last_error<EnsF64>(e); }
NB_API int nbody_ensemble64_set_params(nbody_ensemble64* e, const nbody_params* p) { return ens_set_params<EnsF64>(e, p); }
NB_API int nbody_ensemble64_get_params(const nbody_ensemble64* e, nbody_params* out) { return ens_get_params<EnsF64>(e, out); }
NB_API int nbody_ensemble64_upload(nbody_ensemble64* e, int64_t n_worlds, int64_t n_bodies, const double* pos, const double* vel,
                                   const uint32_t* weight) {
  return ens_upload<EnsF64>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_ensemble64_download(nbody_ensemble64* e, double* pos, double* vel) { return ens_download<EnsF64>(e, pos, vel); }
NB_API int64_t nbody_ensemble64_num_worlds(const nbody_ensemble64* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_ensemble64_num_bodies(const nbody_ensemble64* e) { return e ? e->n_bodies : 0; }
NB_API int nbody_ensemble64_update(nbody_ensemble64* e, double delta, int n_steps, nbody_counting* counter) {
  return ens_update<EnsF64>(e, delta, n_steps, counter);
}
NB_API int nbody_ensemble64_accel(nbody_ensemble64* e, double* acc_xy) { return ens_accel<EnsF64>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_ensemble64(nbody_ensemble64* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  return ens_frames<EnsF64>(e, height, render_px, rgba_out);
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_ensemble64(nbody_ensemble64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                                   uint64_t* step_out) {
  return ens_deltas<EnsF64>(e, flags, out, cap, bytes_out, offsets_out, step_out);
}
// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_sweep_ensemble64(nbody_ensemble64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                                  nbody_counting* counter) {
  return ens_sweep<EnsF64>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_ensemble64(nbody_ensemble64* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<EnsF64>(e, flags, height, ref, out);
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_ensemble64(nbody_ensemble64* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, double* nn_d2,
                                       uint32_t* close) {
  return ens_encounters<EnsF64>(e, flags, limit2, out, nn_index, nn_d2, close);
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_ensemble64(nbody_ensemble64* e, uint32_t flags, double delta, int n_steps, int stride, const float* limit2, uint32_t height,
                                  nbody_world_watch* out, const nbody_watch_rows_f64* rows, nbody_counting* counter) {
  return ens_watch_with<EnsF64>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, WorldRows<EnsF64>(),
                                [e](const EnsF64::Args& a) { return EnsF64::launch(e->stream, e->n_worlds, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_ensemble64(nbody_ensemble64* e, uint32_t flags, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f64* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<EnsF64>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, WorldRows<EnsF64>(),
        [e](const EnsF64::Args& a) { return EnsF64::launch(e->stream, e->n_worlds, a); });
}
// (a resident run — that sweep with every world kept in LDS, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_resident_ensemble64(nbody_ensemble64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                                     nbody_counting* counter) {
  return ens_resident_with<EnsF64>(e, delta, clamp, steps, n_steps, counter);
}
