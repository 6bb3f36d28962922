// libnbody_hip — ragged ensembles in f64: the C entry points of nbody_ragged64_* (include/nbody_ensemble.h) over the driver of
// ragged_driver.h in the precision of ensemble_f64.h, and nbody_ragged64_plan, the plan of ragged_plan.h under the f64 LDS.
#include "ensemble_f64.h"
#include "ragged_driver.h"

using namespace nbody;

struct RagF64 : EnsF64 {
  static constexpr const char* kCreate = "nbody_ragged64_create";
  static constexpr const char* kWho = "ragged";
  static hipError_t launch_items(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, const Ensemble64Args& a) {
    return launch_ensemble64_step_ragged(s, blocks, lds_bytes, items, a);
  }
  static size_t lds_bytes(int n_bodies) { return ensemble64_lds_bytes(n_bodies); }
};
struct nbody_ragged64 : RaggedState<RagF64> {};

NB_API int nbody_ragged64_create(nbody_ragged64** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_ragged64_destroy(nbody_ragged64* e) { ens_destroy(e); }
NB_API const char* nbody_ragged64_last_error(const nbody_ragged64* e) { return ens_last_error<RagF64>(e); }
NB_API int nbody_ragged64_set_params(nbody_ragged64* e, const nbody_params* p) { return ens_set_params<RagF64>(e, p); }
NB_API int nbody_ragged64_get_params(const nbody_ragged64* e, nbody_params* out) { return ens_get_params<RagF64>(e, out); }
NB_API int nbody_ragged64_upload(nbody_ragged64* e, int64_t n_worlds, const int64_t* n_bodies, const double* pos, const double* vel,
                                 const uint32_t* weight) {
  return ragged_upload<RagF64>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_ragged64_download(nbody_ragged64* e, double* pos, double* vel) { return ens_download<RagF64>(e, pos, vel); }
NB_API int64_t nbody_ragged64_num_worlds(const nbody_ragged64* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_ragged64_num_rows(const nbody_ragged64* e) { return e ? e->rows : 0; }
NB_API int nbody_ragged64_sizes(const nbody_ragged64* e, int64_t* n_bodies_out) { return ragged_sizes<RagF64>(e, n_bodies_out); }
NB_API int nbody_ragged64_update(nbody_ragged64* e, double delta, int n_steps, nbody_counting* counter) {
  return ragged_update<RagF64>(e, delta, n_steps, counter);
}
NB_API int nbody_ragged64_accel(nbody_ragged64* e, double* acc_xy) { return ragged_accel<RagF64>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_ragged64(nbody_ragged64* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  return ens_frames<RagF64>(e, height, render_px, rgba_out, ragged_rows<RagF64>(e));
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_ragged64(nbody_ragged64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                                 uint64_t* step_out) {
  return ens_deltas<RagF64>(e, flags, out, cap, bytes_out, offsets_out, step_out, ragged_rows<RagF64>(e));
}

NB_API int nbody_ragged64_plan(int64_t n_worlds, const int64_t* n_bodies, int32_t* launch_of_world, int64_t* first_block_of_world,
                               int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch) {
  // (a refusal is read with nbody_ragged64_last_error(NULL))
  return ragged_show_plan<RagF64>(n_worlds, n_bodies, launch_of_world, first_block_of_world, n_launches, lds_bytes_of_launch, blocks_of_launch);
}

// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: a prefix of its own)
NB_API int nbody_sweep_ragged64(nbody_ragged64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                                nbody_counting* counter) {
  return ragged_sweep<RagF64>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_ragged64(nbody_ragged64* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<RagF64>(e, flags, height, ref, out, ragged_rows<RagF64>(e));
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_ragged64(nbody_ragged64* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, double* nn_d2,
                                     uint32_t* close) {
  return ens_encounters<RagF64>(e, flags, limit2, out, nn_index, nn_d2, close, ragged_rows<RagF64>(e));
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_ragged64(nbody_ragged64* e, uint32_t flags, double delta, int n_steps, int stride, const float* limit2, uint32_t height,
                                nbody_world_watch* out, const nbody_watch_rows_f64* rows, nbody_counting* counter) {
  return ens_watch_with<RagF64>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, ragged_rows<RagF64>(e),
                                [e](const RagF64::Args& a) { return ragged_launch_all<RagF64>(e, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_ragged64(nbody_ragged64* e, uint32_t flags, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f64* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<RagF64>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, ragged_rows<RagF64>(e),
        [e](const RagF64::Args& a) { return ragged_launch_all<RagF64>(e, a); });
}
// (a resident run — that sweep with every world kept in LDS, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_resident_ragged64(nbody_ragged64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                                   nbody_counting* counter) {
  return ragged_resident<RagF64>(e, delta, clamp, steps, n_steps, counter);
}
