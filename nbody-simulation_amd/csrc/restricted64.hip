// libnbody_hip — restricted ensembles in f64: the C entry points of nbody_restricted64_* (include/nbody_ensemble.h), the
// double-precision sibling of restricted.hip.  The bodies are the f64 ensemble's, through the state and the *_with functions of
// ensemble_driver.h in the precision of ensemble_f64.h, stepped by the f64 ensemble's own launch; beside them the handle keeps m
// tracers per world and steps them with the launch of restricted64_kernels.h.  A step is the bodies' launch and then the
// tracers', both given the same Ensemble64Args: the tracers read the buffer the bodies' launch reads (pos_in, the pre-step
// positions — the bodies write the other buffer), and the next step's launches follow in stream order.  Nothing is read back and
// nothing waits between the steps of a call.
#include "ensemble_f64.h"
#include "restricted64_kernels.h"

using namespace nbody;

struct Rst64 : EnsF64 {
  static constexpr const char* kCreate = "nbody_restricted64_create";
  static constexpr const char* kWho = "restricted";
};
struct nbody_restricted64 : EnsembleState<Rst64> {
  int64_t n_tracers = 0;  // per world; 0: none
  double2* tpos = nullptr;
  double2* tvel = nullptr;
  double2* tacc = nullptr;
  ~nbody_restricted64() { drop_tracers(); }  // (ens_destroy has made the device current and drained the stream)
  void drop_tracers() {
    free_dev(tpos); free_dev(tvel); free_dev(tacc);
    n_tracers = 0;
  }
};

namespace {

int rst_fail(nbody_restricted64* e, const char* msg) { return ens_fail<Rst64>(e, NBODY_ERR_INVALID, msg); }
#define RST_HIPCHK(e, call)                                            \
  do {                                                                 \
    hipError_t h__ = (call);                                           \
    if (h__ != hipSuccess) return ens_fail_hip<Rst64>(e, h__, #call);  \
  } while (0)

Restricted64Args rst_tracers(const nbody_restricted64* e) {
  Restricted64Args t;
  t.tpos = e->tpos;
  t.n_tracers = e->n_tracers;
  return t;
}

}  // namespace

NB_API int nbody_restricted64_create(nbody_restricted64** out, int device_id) { return ens_create(out, device_id); }
NB_API void nbody_restricted64_destroy(nbody_restricted64* e) { ens_destroy(e); }
NB_API const char* nbody_restricted64_last_error(const nbody_restricted64* e) { return ens_last_error<Rst64>(e); }
NB_API int nbody_restricted64_set_params(nbody_restricted64* e, const nbody_params* p) { return ens_set_params<Rst64>(e, p); }
NB_API int nbody_restricted64_get_params(const nbody_restricted64* e, nbody_params* out) { return ens_get_params<Rst64>(e, out); }

NB_API int nbody_restricted64_upload(nbody_restricted64* e, int64_t n_worlds, int64_t n_bodies, const double* pos, const double* vel,
                                     const uint32_t* weight) {
  if (!e) return NBODY_ERR_INVALID;
  if (n_bodies < 1 || n_bodies > kEnsembleMaxBodies)
    return rst_fail(e, "restricted upload: n_bodies must be 1 .. 4096 (above that a context per world is the tool)");
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows / n_bodies)
    return rst_fail(e, "restricted upload: n_worlds must be >= 1 and n_worlds * n_bodies <= 2^26");
  if (!pos || !vel) return rst_fail(e, "restricted upload: pos_xy or vel_xy is NULL");
  if (int rc = ens_store_rows<Rst64>(e, n_worlds * n_bodies, pos, vel, weight)) {  // (drains the stream before it frees)
    e->drop_tracers();
    return rc;
  }
  e->drop_tracers();  // a new world
  e->n_worlds = n_worlds;
  e->n_bodies = n_bodies;
  return NBODY_OK;
}
NB_API int nbody_restricted64_download(nbody_restricted64* e, double* pos, double* vel) { return ens_download<Rst64>(e, pos, vel); }
NB_API int64_t nbody_restricted64_num_worlds(const nbody_restricted64* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_restricted64_num_bodies(const nbody_restricted64* e) { return e ? e->n_bodies : 0; }
NB_API int64_t nbody_restricted64_num_tracers(const nbody_restricted64* e) { return e ? e->n_tracers : 0; }

NB_API int nbody_restricted64_tracers_upload(nbody_restricted64* e, int64_t n_worlds, int64_t n_tracers, const double* pos, const double* vel) {
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
  const size_t bytes = (size_t)(n_worlds * n_tracers) * sizeof(double2);
  hipError_t h = hipMalloc((void**)&e->tpos, bytes);
  if (h == hipSuccess) h = hipMalloc((void**)&e->tvel, bytes);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tpos, pos, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tvel, vel, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    e->drop_tracers();
    return ens_fail_hip<Rst64>(e, h, "upload of the tracers");
  }
  e->n_tracers = n_tracers;
  return NBODY_OK;
}

NB_API int nbody_restricted64_tracers_download(nbody_restricted64* e, double* pos, double* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_download: nothing uploaded");
  if (!e->n_tracers) return NBODY_OK;
  RST_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_tracers) * sizeof(double2);
  if (pos) RST_HIPCHK(e, hipMemcpyAsync(pos, e->tpos, bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) RST_HIPCHK(e, hipMemcpyAsync(vel, e->tvel, bytes, hipMemcpyDeviceToHost, e->stream));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

NB_API int nbody_restricted64_update(nbody_restricted64* e, double delta, int n_steps, nbody_counting* counter) {
  return ens_update_with<Rst64>(e, delta, n_steps, counter, [e](const Ensemble64Args& a) {
    hipError_t h = launch_ensemble64_step(e->stream, e->n_worlds, a);
    if (h != hipSuccess || !e->n_tracers) return h;
    Restricted64Args t = rst_tracers(e);
    t.tvel = e->tvel;
    return launch_restricted64_tracers(e->stream, e->n_worlds, a, t);  // a.pos_in: what the bodies' launch above reads
  });
}

NB_API int nbody_restricted64_accel(nbody_restricted64* e, double* acc_xy) {
  return ens_accel_with<Rst64>(e, acc_xy, [e](const Ensemble64Args& a) { return launch_ensemble64_step(e->stream, e->n_worlds, a); });
}

NB_API int nbody_restricted64_tracers_accel(nbody_restricted64* e, double* acc_xy) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_accel: nothing uploaded");
  if (!e->n_tracers) return NBODY_OK;
  if (!acc_xy) return rst_fail(e, "restricted tracers_accel: acc_xy is NULL");
  RST_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_tracers) * sizeof(double2);
  if (!e->tacc) RST_HIPCHK(e, hipMalloc((void**)&e->tacc, bytes));
  Restricted64Args t = rst_tracers(e);
  t.tacc_out = e->tacc;
  RST_HIPCHK(e, launch_restricted64_tracers(e->stream, e->n_worlds, ens_args<Rst64>(e), t));
  RST_HIPCHK(e, hipMemcpyAsync(acc_xy, e->tacc, bytes, hipMemcpyDeviceToHost, e->stream));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}
