// libnbody_hip — ensembles: the C entry points of nbody_ensemble_* (include/nbody_hip.h) over the driver of ensemble_driver.h
// in the precision of ensemble_f32.h.
#include "ensemble_f32.h"

using namespace nbody;

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
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_ensemble(nbody_ensemble* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  return ens_frames<EnsF32>(e, height, render_px, rgba_out);
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_ensemble(nbody_ensemble* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                                 uint64_t* step_out) {
  return ens_deltas<EnsF32>(e, flags, out, cap, bytes_out, offsets_out, step_out);
}
// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_sweep_ensemble(nbody_ensemble* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                                nbody_counting* counter) {
  return ens_sweep<EnsF32>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_ensemble(nbody_ensemble* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<EnsF32>(e, flags, height, ref, out);
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_ensemble(nbody_ensemble* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, float* nn_d2,
                                     uint32_t* close) {
  return ens_encounters<EnsF32>(e, flags, limit2, out, nn_index, nn_d2, close);
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_ensemble(nbody_ensemble* e, uint32_t flags, float delta, int n_steps, int stride, const float* limit2, uint32_t height,
                                nbody_world_watch* out, const nbody_watch_rows_f32* rows, nbody_counting* counter) {
  return ens_watch_with<EnsF32>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, WorldRows<EnsF32>(),
                                [e](const EnsF32::Args& a) { return EnsF32::launch(e->stream, e->n_worlds, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_ensemble(nbody_ensemble* e, uint32_t flags, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f32* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<EnsF32>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, WorldRows<EnsF32>(),
        [e](const EnsF32::Args& a) { return EnsF32::launch(e->stream, e->n_worlds, a); });
}
// (what such a call samples, and in how many launches: pure host code, no handle)
NB_API int nbody_wsweep_plan(int64_t n_worlds, const int32_t* steps, int n_steps, const int32_t* stride, uint32_t flags, int64_t* samples_of_world,
                             int64_t* n_sampling_launches) {
  return wsweep_show_plan(n_worlds, steps, n_steps, stride, flags, samples_of_world, n_sampling_launches);
}
// (a resident run — that sweep with every world kept in LDS, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_resident_ensemble(nbody_ensemble* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                                   nbody_counting* counter) {
  return ens_resident_with<EnsF32>(e, delta, clamp, steps, n_steps, counter);
}
// (its launches and their dynamic LDS: pure host code, no handle)
static_assert(NBODY_RESIDENT_MAX_BODIES == kResidentMaxBodies && NBODY_RESIDENT_STEPS_PER_LAUNCH == kResidentStepsPerLaunch,
              "the header's constants are the kernels'");
NB_API int nbody_resident_plan(int64_t n_worlds, const int64_t* n_bodies, const int32_t* steps, int n_steps, int is_f64, int32_t* n_launches,
                               int32_t* lds_bytes) {
  return resident_plan(n_worlds, n_bodies, steps, n_steps, is_f64, n_launches, lds_bytes) ? NBODY_ERR_INVALID : NBODY_OK;
}
