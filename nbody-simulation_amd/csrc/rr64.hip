// libnbody_hip — ragged restricted ensembles in f64: the C entry points of nbody_rr64_* (include/nbody_ensemble.h) over the
// driver of rr_driver.h in the precision of ensemble_f64.h, with the bodies' launch of ensemble64_kernels.h and the tracers'
// launch of rr64_kernels.h, and nbody_rr64_plan, the tracers' plan of rr_plan.h under the f64 LDS.
#include "ensemble_f64.h"
#include "rr64_kernels.h"
#include "rr_driver.h"

using namespace nbody;

static_assert(NBODY_RR_MAX_LAUNCHES == 2 * kRaggedMaxLaunches, "the header's constant: the bodies' launches and the tracers'");
static_assert(sizeof(RaggedItem) == sizeof(uint2), "a work item of the bodies is the device's uint2");
static_assert(sizeof(RrItem) == sizeof(uint4), "a work item of the tracers is the device's uint4");
// (the plan's 512-tracer tile serves both precisions only because both per-lane counts are 2)
static_assert(kRrTile == kEnsembleBlock * kRestricted64PerLane, "the plan's tile is the f64 kernel's");

struct RrF64 : EnsF64 {
  using Tracers = Rr64TracerArgs;
  static constexpr const char* kCreate = "nbody_rr64_create";
  static constexpr const char* kWho = "ragged restricted";
  static hipError_t launch_items(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, const Ensemble64Args& a) {
    return launch_ensemble64_step_ragged(s, blocks, lds_bytes, items, a);
  }
  static hipError_t launch_tracer_items(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint4* items, const Ensemble64Args& a,
                                        const Rr64TracerArgs& t) {
    return launch_rr64_tracers(s, blocks, lds_bytes, items, a, t);
  }
  static size_t lds_bytes(int n_bodies) { return ensemble64_lds_bytes(n_bodies); }
};
struct nbody_rr64 : RrState<RrF64> {};

NB_API int nbody_rr64_create(nbody_rr64** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_rr64_destroy(nbody_rr64* e) { ens_destroy(e); }
NB_API const char* nbody_rr64_last_error(const nbody_rr64* e) { return ens_last_error<RrF64>(e); }
NB_API int nbody_rr64_set_params(nbody_rr64* e, const nbody_params* p) { return ens_set_params<RrF64>(e, p); }
NB_API int nbody_rr64_get_params(const nbody_rr64* e, nbody_params* out) { return ens_get_params<RrF64>(e, out); }
NB_API int nbody_rr64_upload(nbody_rr64* e, int64_t n_worlds, const int64_t* n_bodies, const double* pos, const double* vel,
                             const uint32_t* weight) {
  return rr_upload<RrF64>(e, n_worlds, n_bodies, pos, vel, weight);
}
NB_API int nbody_rr64_download(nbody_rr64* e, double* pos, double* vel) { return ens_download<RrF64>(e, pos, vel); }
NB_API int nbody_rr64_tracers_upload(nbody_rr64* e, int64_t n_worlds, const int64_t* n_tracers, const double* pos, const double* vel) {
  return rr_tracers_upload<RrF64>(e, n_worlds, n_tracers, pos, vel);
}
NB_API int nbody_rr64_tracers_download(nbody_rr64* e, double* pos, double* vel) { return rr_tracers_download<RrF64>(e, pos, vel); }
NB_API int64_t nbody_rr64_num_worlds(const nbody_rr64* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_rr64_num_rows(const nbody_rr64* e) { return e ? e->rows : 0; }
NB_API int64_t nbody_rr64_num_tracer_rows(const nbody_rr64* e) { return e ? e->tracer_rows : 0; }
NB_API int nbody_rr64_sizes(const nbody_rr64* e, int64_t* n_bodies_out, int64_t* n_tracers_out) {
  return rr_sizes<RrF64>(e, n_bodies_out, n_tracers_out);
}
NB_API int nbody_rr64_update(nbody_rr64* e, double delta, int n_steps, nbody_counting* counter) {
  return rr_update<RrF64>(e, delta, n_steps, counter);
}
NB_API int nbody_rr64_accel(nbody_rr64* e, double* acc_xy) { return rr_accel<RrF64>(e, acc_xy); }
NB_API int nbody_rr64_tracers_accel(nbody_rr64* e, double* acc_xy) { return rr_tracers_accel<RrF64>(e, acc_xy); }
// (frames of every world, ensemble_frames.h: a prefix of its own, defined here where the handle is a complete type)
NB_API int nbody_frames_rr64(nbody_rr64* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out) {
  return ens_frames<RrF64>(e, height, render_px, rgba_out, rr_rows<RrF64>(e), with_tracers != 0);
}
// (delta streams of every world, ensemble_deltas.h: likewise a prefix of its own)
NB_API int nbody_deltas_rr64(nbody_rr64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                             uint64_t* step_out) {
  return ens_deltas<RrF64>(e, flags, out, cap, bytes_out, offsets_out, step_out, rr_rows<RrF64>(e));
}

NB_API int nbody_rr64_plan(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, int32_t* launch_of_world,
                           int64_t* first_block_of_world, int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch) {
  // (a refusal is read with nbody_rr64_last_error(NULL))
  return rr_show_plan<RrF64>(n_worlds, n_bodies, n_tracers, launch_of_world, first_block_of_world, n_launches, lds_bytes_of_launch,
                             blocks_of_launch);
}

// (a sweep — a time step, a clamp and a number of steps per world, include/nbody_ensemble.h: a prefix of its own)
NB_API int nbody_sweep_rr64(nbody_rr64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                            nbody_counting* counter) {
  return rr_sweep<RrF64>(e, delta, clamp, steps, n_steps, counter);
}
// (a record per world — moments, extent, separations, ensemble_summary.h: likewise a prefix of its own)
NB_API int nbody_summary_rr64(nbody_rr64* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out) {
  return ens_summary<RrF64>(e, flags, height, ref, out, rr_rows<RrF64>(e));
}
// (nearest neighbours and clamped pairs per world, ensemble_encounters.h: likewise a prefix of its own)
NB_API int nbody_encounters_rr64(nbody_rr64* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index, double* nn_d2,
                                 uint32_t* close) {
  return ens_encounters<RrF64>(e, flags, limit2, out, nn_index, nn_d2, close, rr_rows<RrF64>(e));
}
// (an update sampled before, between and after its steps, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_watch_rr64(nbody_rr64* e, uint32_t flags, double delta, int n_steps, int stride, const float* limit2, uint32_t height,
                            nbody_world_watch* out, const nbody_watch_rows_f64* rows, nbody_counting* counter) {
  return ens_watch_with<RrF64>(e, flags, delta, n_steps, stride, limit2, height, out, rows, counter, rr_rows<RrF64>(e),
                               [e](const RrF64::Args& a) { return rr_launch_step<RrF64>(e, a); });
}
// (a sweep sampled on every world's own schedule, ensemble_watch.h: likewise a prefix of its own)
NB_API int nbody_wsweep_rr64(nbody_rr64* e, uint32_t flags, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
        const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out, const nbody_watch_rows_f64* rows,
        nbody_counting* counter) {
  return ens_wsweep_with<RrF64>(e, flags, delta, clamp, steps, n_steps, stride, limit2, height, out, rows, counter, rr_rows<RrF64>(e),
        [e](const RrF64::Args& a) { return rr_launch_step<RrF64>(e, a); });
}
