// libnbody_hip — restricted ensembles: the C entry points of nbody_restricted_* (include/nbody_ensemble.h).  The bodies are the
// ensemble's, through the state and the *_with functions of ensemble_driver.h in the precision of ensemble_f32.h, stepped by the
// ensemble's own launch; beside them the handle keeps m tracers per world and steps them with the launch of restricted_kernels.h.
// A step is the bodies' launch and then the tracers', both given the same EnsembleArgs: the tracers read the buffer the bodies'
// launch reads (pos_in, the pre-step positions — the bodies write the other buffer), and the next step's launches follow in
// stream order.  Nothing is read back and nothing waits between the steps of a call.
#include "ensemble_f32.h"
#include "restricted_kernels.h"

using namespace nbody;

struct RstF32 : EnsF32 {
  static constexpr const char* kCreate = "nbody_restricted_create";
  static constexpr const char* kWho = "restricted";
};
struct nbody_restricted : EnsembleState<RstF32> {
  int64_t n_tracers = 0;  // per world; 0: none
  float2* tpos = nullptr;
  float2* tvel = nullptr;
  float2* tacc = nullptr;
  ~nbody_restricted() { drop_tracers(); }  // (ens_destroy has made the device current and drained the stream)
  void drop_tracers() {
    free_dev(tpos); free_dev(tvel); free_dev(tacc);
    n_tracers = 0;
  }
};

namespace {

int rst_fail(nbody_restricted* e, const char* msg) { return ens_fail<RstF32>(e, NBODY_ERR_INVALID, msg); }
#define RST_HIPCHK(e, call)                                             \
  do {                                                                  \
    hipError_t h__ = (call);                                            \
    if (h__ != hipSuccess) return ens_fail_hip<RstF32>(e, h__, #call);  \
  } while (0)

RestrictedArgs rst_tracers(const nbody_restricted* e) {
  RestrictedArgs t;
  t.tpos = e->tpos;
  t.n_tracers = e->n_tracers;
  return t;
}

}  // namespace

NB_API int nbody_restricted_create(nbody_restricted** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_restricted_destroy(nbody_restricted* e) { ens_destroy(e); }
NB_API const char* nbody_restricted_last_error(const nbody_restricted* e) { return ens_last_error<RstF32>(e); }
NB_API int nbody_restricted_set_params(nbody_restricted* e, const nbody_params* p) { return ens_set_params<RstF32>(e, p); }
NB_API int nbody_restricted_get_params(const nbody_restricted* e, nbody_params* out) { return ens_get_params<RstF32>(e, out); }

NB_API int nbody_restricted_upload_f32(nbody_restricted* e, int64_t n_worlds, int64_t n_bodies, const float* pos, const float* vel,
                                       const uint32_t* weight) {
  if (!e) return NBODY_ERR_INVALID;
  if (n_bodies < 1 || n_bodies > kEnsembleMaxBodies)
    return rst_fail(e, "restricted upload: n_bodies must be 1 .. 4096 (above that a context per world is the tool)");
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows / n_bodies)
    return rst_fail(e, "restricted upload: n_worlds must be >= 1 and n_worlds * n_bodies <= 2^26");
  if (!pos || !vel) return rst_fail(e, "restricted upload: pos_xy or vel_xy is NULL");
  if (int rc = ens_store_rows<RstF32>(e, n_worlds * n_bodies, pos, vel, weight)) {  // (drains the stream before it frees)
    e->drop_tracers();
    return rc;
  }
  e->drop_tracers();  // a new world
  e->n_worlds = n_worlds;
  e->n_bodies = n_bodies;
  return NBODY_OK;
}
NB_API int nbody_restricted_download_f32(nbody_restricted* e, float* pos, float* vel) { return ens_download<RstF32>(e, pos, vel); }
NB_API int64_t nbody_restricted_num_worlds(const nbody_restricted* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_restricted_num_bodies(const nbody_restricted* e) { return e ? e->n_bodies : 0; }
NB_API int64_t nbody_restricted_num_tracers(const nbody_restricted* e) { return e ? e->n_tracers : 0; }

NB_API int nbody_restricted_tracers_upload_f32(nbody_restricted* e, int64_t n_worlds, int64_t n_tracers, const float* pos, const float* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_upload: nothing uploaded (the bodies come first)");
  if (n_worlds != e->n_worlds) return rst_fail(e, "restricted tracers_upload: n_worlds is not the number of worlds of the bodies");
  if (n_tracers < 0 || n_tracers > kEnsembleMaxRows / n_worlds)
    return rst_fail(e, "restricted tracers_upload: n_tracers must be >= 0 and n_worlds * n_tracers <= 2^26");
  if (n_tracers > 0 && (!pos || !vel)) return rst_fail(e, "restricted tracers_upload: pos_xy or vel_xy is NULL");
  RST_HIPCHK(e, hipSetDevice(e->device));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  e->drop_tracers();
  if (n_tracers == 0) return NBODY_OK;
  const size_t bytes = (size_t)(n_worlds * n_tracers) * sizeof(float2);
  hipError_t h = hipMalloc((void**)&e->tpos, bytes);
  if (h == hipSuccess) h = hipMalloc((void**)&e->tvel, bytes);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tpos, pos, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tvel, vel, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    e->drop_tracers();
    return ens_fail_hip<RstF32>(e, h, "upload of the tracers");
  }
  e->n_tracers = n_tracers;
  return NBODY_OK;
}

NB_API int nbody_restricted_tracers_download_f32(nbody_restricted* e, float* pos, float* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_download: nothing uploaded");
  if (!e->n_tracers) return NBODY_OK;
  RST_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_tracers) * sizeof(float2);
  if (pos) RST_HIPCHK(e, hipMemcpyAsync(pos, e->tpos, bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) RST_HIPCHK(e, hipMemcpyAsync(vel, e->tvel, bytes, hipMemcpyDeviceToHost, e->stream));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

NB_API int nbody_restricted_update_f32(nbody_restricted* e, float delta, int n_steps, nbody_counting* counter) {
  return ens_update_with<RstF32>(e, delta, n_steps, counter, [e](const EnsembleArgs& a) {
    hipError_t h = launch_ensemble_step(e->stream, e->n_worlds, a);
    if (h != hipSuccess || !e->n_tracers) return h;
    RestrictedArgs t = rst_tracers(e);
    t.tvel = e->tvel;
    return launch_restricted_tracers(e->stream, e->n_worlds, a, t);  // a.pos_in: what the bodies' launch above reads
  });
}

NB_API int nbody_restricted_accel_f32(nbody_restricted* e, float* acc_xy) {
  return ens_accel_with<RstF32>(e, acc_xy, [e](const EnsembleArgs& a) { return launch_ensemble_step(e->stream, e->n_worlds, a); });
}

NB_API int nbody_restricted_tracers_accel_f32(nbody_restricted* e, float* acc_xy) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_accel: nothing uploaded");
  if (!e->n_tracers) return NBODY_OK;
  if (!acc_xy) return rst_fail(e, "restricted tracers_accel: acc_xy is NULL");
  RST_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_tracers) * sizeof(float2);
  if (!e->tacc) RST_HIPCHK(e, hipMalloc((void**)&e->tacc, bytes));
  RestrictedArgs t = rst_tracers(e);
  t.tacc_out = e->tacc;
  RST_HIPCHK(e, launch_restricted_tracers(e->stream, e->n_worlds, ens_args<RstF32>(e), t));
  RST_HIPCHK(e, hipMemcpyAsync(acc_xy, e->tacc, bytes, hipMemcpyDeviceToHost, e->stream));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}
