// libnbody_hip — ragged ensembles: the C entry points of nbody_ragged_* (include/nbody_ensemble.h) over the driver of
// ragged_driver.h in the precision of ensemble_f32.h, and nbody_ragged_plan, the plan of ragged_plan.h as the ABI shows it.
#include "ensemble_f32.h"
#include "ragged_driver.h"

using namespace nbody;

static_assert(NBODY_RAGGED_MAX_LAUNCHES == kRaggedMaxLaunches, "the header's constant is the plan's");
static_assert(sizeof(RaggedItem) == sizeof(uint2), "a work item is the device's uint2");

struct RagF32 : EnsF32 {
  static constexpr const char* kCreate = "nbody_ragged_create";
  static constexpr const char* kWho = "ragged";
  static hipError_t launch_items(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, const EnsembleArgs& a) {
    return launch_ensemble_step_ragged(s, blocks, lds_bytes, items, a);
  }
  static size_t lds_bytes(int n_bodies) { return ensemble_lds_bytes(n_bodies); }
};
struct nbody_ragged : RaggedState<RagF32> {};

NB_API int nbody_ragged_create(nbody_ragged** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_ragged_destroy(nbody_ragged* e) { ens_destroy(e); }
NB_API const char* nbody_ragged_last_error(const nbody_ragged* e) { return ens_last_error<RagF32>(e); }
NB_API int nbody_ragged_set_params(nbody_ragged* e, const nbody_params* p) { return ens_set_params<RagF32>(e, p); }
NB_API int nbody_ragged_get_params(const nbody_ragged* e, nbody_params* out) { return ens_get_params<RagF32>(e, out); }
NB_API int nbody_ragged_upload_f32(nbody_ragged* e, int64_t n_worlds, const int64_t* n_bodies, const float* pos, const float* vel,
                                   const uint32_t* weight) {
  return ragged_upload<RagF32>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_ragged_download_f32(nbody_ragged* e, float* pos, float* vel) { return ens_download<RagF32>(e, pos, vel); }
NB_API int64_t nbody_ragged_num_worlds(const nbody_ragged* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_ragged_num_rows(const nbody_ragged* e) { return e ? e->rows : 0; }
NB_API int nbody_ragged_sizes(const nbody_ragged* e, int64_t* n_bodies_out) { return ragged_sizes<RagF32>(e, n_bodies_out); }
NB_API int nbody_ragged_update_f32(nbody_ragged* e, float delta, int n_steps, nbody_counting* counter) {
  return ragged_update<RagF32>(e, delta, n_steps, counter);
}
NB_API int nbody_ragged_accel_f32(nbody_ragged* e, float* acc_xy) { return ragged_accel<RagF32>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_ragged(nbody_ragged* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  return ens_frames<RagF32>(e, height, render_px, rgba_out, ragged_rows<RagF32>(e));
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_ragged(nbody_ragged* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                               uint64_t* step_out) {
  return ens_deltas<RagF32>(e, flags, out, cap, bytes_out, offsets_out, step_out, ragged_rows<RagF32>(e));
}

NB_API int nbody_ragged_plan(int64_t n_worlds, const int64_t* n_bodies, int32_t* launch_of_world, int64_t* first_block_of_world,
                             int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch) {
  // (a refusal is read with nbody_ragged_last_error(NULL))
  return ragged_show_plan<RagF32>(n_worlds, n_bodies, launch_of_world, first_block_of_world, n_launches, lds_bytes_of_launch, blocks_of_launch);
}

// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: a prefix of its own)
NB_API int nbody_sweep_ragged(nbody_ragged* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                              nbody_counting* counter) {
  return ragged_sweep<RagF32>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_ragged(nbody_ragged* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<RagF32>(e, flags, height, ref, out, ragged_rows<RagF32>(e));
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_ragged(nbody_ragged* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, float* nn_d2,
                                   uint32_t* close) {
  return ens_encounters<RagF32>(e, flags, limit2, out, nn_index, nn_d2, close, ragged_rows<RagF32>(e));
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_ragged(nbody_ragged* e, uint32_t flags, float delta, int n_steps, int stride, const float* limit2, uint32_t height,
                              nbody_world_watch* out, const nbody_watch_rows_f32* rows, nbody_counting* counter) {
  return ens_watch_with<RagF32>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, ragged_rows<RagF32>(e),
                                [e](const RagF32::Args& a) { return ragged_launch_all<RagF32>(e, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_ragged(nbody_ragged* e, uint32_t flags, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f32* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<RagF32>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, ragged_rows<RagF32>(e),
        [e](const RagF32::Args& a) { return ragged_launch_all<RagF32>(e, a); });
}
// (a resident run — that sweep with every world kept in LDS, include/nbody_ensemble.h: likewise a prefix of its own)
NB_API int nbody_resident_ragged(nbody_ragged* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                                 nbody_counting* counter) {
  return ragged_resident<RagF32>(e, delta, clamp, steps, n_steps, counter);
}
