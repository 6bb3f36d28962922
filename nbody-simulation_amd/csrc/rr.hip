// libnbody_hip — ragged restricted ensembles: the C entry points of nbody_rr_* (include/nbody_ensemble.h) over the driver of
// rr_driver.h in the precision of ensemble_f32.h, with the bodies' launch of ensemble_kernels.h and the tracers' launch of
// rr_kernels.h, and nbody_rr_plan, the tracers' plan of rr_plan.h as the ABI shows it.
#include "ensemble_f32.h"
#include "rr_driver.h"
#include "rr_kernels.h"

using namespace nbody;

static_assert(NBODY_RR_MAX_LAUNCHES == 2 * kRaggedMaxLaunches, "the header's constant: the bodies' launches and the tracers'");
static_assert(sizeof(RaggedItem) == sizeof(uint2), "a work item of the bodies is the device's uint2");
static_assert(sizeof(RrItem) == sizeof(uint4), "a work item of the tracers is the device's uint4");
static_assert(kRrTile == kEnsembleBlock * kRestrictedPerLane, "the plan's tile is the kernel's");

struct RrF32 : EnsF32 {
  using Tracers = RrTracerArgs;
  static constexpr const char* kCreate = "nbody_rr_create";
  static constexpr const char* kWho = "ragged restricted";
  static hipError_t launch_items(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, const EnsembleArgs& a) {
    return launch_ensemble_step_ragged(s, blocks, lds_bytes, items, a);
  }
  static hipError_t launch_tracer_items(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint4* items, const EnsembleArgs& a,
                                        const RrTracerArgs& t) {
    return launch_rr_tracers(s, blocks, lds_bytes, items, a, t);
  }
  static size_t lds_bytes(int n_bodies) { return ensemble_lds_bytes(n_bodies); }
};
struct nbody_rr : RrState<RrF32> {};

NB_API int nbody_rr_create(nbody_rr** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_rr_destroy(nbody_rr* e) { ens_destroy(e); }
NB_API const char* nbody_rr_last_error(const nbody_rr* e) { return ens_last_error<RrF32>(e); }
NB_API int nbody_rr_set_params(nbody_rr* e, const nbody_params* p) { return ens_set_params<RrF32>(e, p); }
NB_API int nbody_rr_get_params(const nbody_rr* e, nbody_params* out) { return ens_get_params<RrF32>(e, out); }
NB_API int nbody_rr_upload_f32(nbody_rr* e, int64_t n_worlds, const int64_t* n_bodies, const float* pos, const float* vel,
                               const uint32_t* weight) {
  return rr_upload<RrF32>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_rr_download_f32(nbody_rr* e, float* pos, float* vel) { return ens_download<RrF32>(e, pos, vel); }
NB_API int nbody_rr_tracers_upload_f32(nbody_rr* e, int64_t n_worlds, const int64_t* n_tracers, const float* pos, const float* vel) {
  return rr_tracers_upload<RrF32>(e, n_worlds, n_tracers, pos, vel);
}
NB_API int nbody_rr_tracers_download_f32(nbody_rr* e, float* pos, float* vel) { return rr_tracers_download<RrF32>(e, pos, vel); }
NB_API int64_t nbody_rr_num_worlds(const nbody_rr* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_rr_num_rows(const nbody_rr* e) { return e ? e->rows : 0; }
NB_API int64_t nbody_rr_num_tracer_rows(const nbody_rr* e) { return e ? e->tracer_rows : 0; }
NB_API int nbody_rr_sizes(const nbody_rr* e, int64_t* n_bodies_out, int64_t* n_tracers_out) {
  return rr_sizes<RrF32>(e, n_bodies_out, n_tracers_out);
}
NB_API int nbody_rr_update_f32(nbody_rr* e, float delta, int n_steps, nbody_counting* counter) {
  return rr_update<RrF32>(e, delta, n_steps, counter);
}
NB_API int nbody_rr_accel_f32(nbody_rr* e, float* acc_xy) { return rr_accel<RrF32>(e, acc_xy); }
NB_API int nbody_rr_tracers_accel_f32(nbody_rr* e, float* acc_xy) { return rr_tracers_accel<RrF32>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_rr(nbody_rr* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out) {
  return ens_frames<RrF32>(e, height, render_px, rgba_out, rr_rows<RrF32>(e), with_tracers != 0);
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_rr(nbody_rr* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                           uint64_t* step_out) {
  return ens_deltas<RrF32>(e, flags, out, cap, bytes_out, offsets_out, step_out, rr_rows<RrF32>(e));
}

NB_API int nbody_rr_plan(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, int32_t* launch_of_world,
                         int64_t* first_block_of_world, int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch) {
  // (a refusal is read with nbody_rr_last_error(NULL))
  return rr_show_plan<RrF32>(n_worlds, n_bodies, n_tracers, launch_of_world, first_block_of_world, n_launches, lds_bytes_of_launch,
                             blocks_of_launch);
}

// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: a prefix of its own)
NB_API int nbody_sweep_rr(nbody_rr* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                          nbody_counting* counter) {
  return rr_sweep<RrF32>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_rr(nbody_rr* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<RrF32>(e, flags, height, ref, out, rr_rows<RrF32>(e));
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_rr(nbody_rr* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, float* nn_d2,
                               uint32_t* close) {
  return ens_encounters<RrF32>(e, flags, limit2, out, nn_index, nn_d2, close, rr_rows<RrF32>(e));
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_rr(nbody_rr* e, uint32_t flags, float delta, int n_steps, int stride, const float* limit2, uint32_t height,
                          nbody_world_watch* out, const nbody_watch_rows_f32* rows, nbody_counting* counter) {
  return ens_watch_with<RrF32>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, rr_rows<RrF32>(e),
                               [e](const RrF32::Args& a) { return rr_launch_step<RrF32>(e, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_rr(nbody_rr* e, uint32_t flags, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f32* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<RrF32>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, rr_rows<RrF32>(e),
        [e](const RrF32::Args& a) { return rr_launch_step<RrF32>(e, a); });
}
