// libnbody_hip — ensembles: the handle and the C entry points of nbody_ensemble_* (include/nbody_hip.h).  Many worlds of one
// size in world-major device arrays, every step of all of them one launch of ensemble_kernels.hip on the handle's stream.
// The positions are double-buffered across steps (a world's other blocks still read the old ones), velocities are updated in
// place.  No CPU path and no host synchronisation between the steps of a call.
#include <new>
#include <vector>

#include "driver.h"
#include "ensemble_host.h"
#include "ensemble_kernels.h"

using namespace nbody;

struct nbody_ensemble {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  nbody_params params{};
  nbody_counting counting{};
  int64_t n_worlds = 0, n_bodies = 0;  // 0: nothing uploaded
  float2* pos[2] = {nullptr, nullptr};
  int cur = 0;
  float2* vel = nullptr;
  float* mass = nullptr;
  float2* acc = nullptr;
};

namespace {

thread_local std::string g_ens_create_error;

int ens_fail(nbody_ensemble* e, int code, const std::string& msg) {
  if (e) e->err = msg; else g_ens_create_error = msg;
  return code;
}
int ens_fail_hip(nbody_ensemble* e, hipError_t h, const char* what) {
  return ens_fail(e, NBODY_ERR_HIP, std::string("ensemble: ") + what + ": " + hipGetErrorString(h));
}
#define ENS_HIPCHK(e, call)                                     \
  do {                                                          \
    hipError_t h__ = (call);                                    \
    if (h__ != hipSuccess) return ens_fail_hip(e, h__, #call);  \
  } while (0)

void ens_free(nbody_ensemble* e) {
  free_dev(e->pos[0]); free_dev(e->pos[1]); free_dev(e->vel); free_dev(e->mass); free_dev(e->acc);
  e->n_worlds = e->n_bodies = 0;
  e->cur = 0;
}

EnsembleArgs ens_args(const nbody_ensemble* e) {
  EnsembleArgs a;
  a.pos_in = e->pos[e->cur];
  a.mass = e->mass;
  a.n_bodies = (int)e->n_bodies;
  a.clamp = e->params.clamp;
  a.arith = direct_arith_f32(e->params.arith, e->params.clamp);  // a clamp below kFastClampFloor (or NaN): every world EXACT
  return a;
}

}  // namespace

NB_API int nbody_ensemble_create(nbody_ensemble** out, int device_id) {
  if (!out) return ens_fail(nullptr, NBODY_ERR_INVALID, "nbody_ensemble_create: out is NULL");
  *out = nullptr;
  hipStream_t stream = nullptr;
  std::string msg;
  const int rc = ensemble_open_device("nbody_ensemble_create", device_id, &stream, msg);
  if (rc != NBODY_OK) return ens_fail(nullptr, rc, msg);
  nbody_ensemble* e = new (std::nothrow) nbody_ensemble();
  if (!e) {
    ensemble_close_stream(stream);
    return ens_fail(nullptr, NBODY_ERR_NOMEM, "nbody_ensemble_create: out of host memory");
  }
  e->device = device_id;
  e->stream = stream;
  nbody_default_params(&e->params);
  *out = e;
  return NBODY_OK;
}

NB_API void nbody_ensemble_destroy(nbody_ensemble* e) {
  if (!e) return;
  ensemble_drain(e->device, e->stream);
  ens_free(e);
  ensemble_close_stream(e->stream);
  delete e;
}

NB_API const char* nbody_ensemble_last_error(const nbody_ensemble* e) { return e ? e->err.c_str() : g_ens_create_error.c_str(); }

NB_API int nbody_ensemble_set_params(nbody_ensemble* e, const nbody_params* p) {
  if (!e || !p) return NBODY_ERR_INVALID;
  if (p->arith < NBODY_ARITH_AUTO || p->arith > NBODY_ARITH_EXACT) return ens_fail(e, NBODY_ERR_INVALID, "ensemble set_params: bad arith");
  e->params = *p;
  return NBODY_OK;
}
NB_API int nbody_ensemble_get_params(const nbody_ensemble* e, nbody_params* out) {
  if (!e || !out) return NBODY_ERR_INVALID;
  *out = e->params;
  return NBODY_OK;
}

NB_API int nbody_ensemble_upload_f32(nbody_ensemble* e, int64_t n_worlds, int64_t n_bodies, const float* pos, const float* vel,
                                     const uint32_t* weight) {
  if (!e) return NBODY_ERR_INVALID;
  if (n_bodies < 1 || n_bodies > kEnsembleMaxBodies)
    return ens_fail(e, NBODY_ERR_INVALID, "ensemble upload: n_bodies must be 1 .. 4096 (above that a context per world is the tool)");
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows / n_bodies)
    return ens_fail(e, NBODY_ERR_INVALID, "ensemble upload: n_worlds must be >= 1 and n_worlds * n_bodies <= 2^26");
  if (!pos || !vel) return ens_fail(e, NBODY_ERR_INVALID, "ensemble upload: pos_xy or vel_xy is NULL");
  ENS_HIPCHK(e, hipSetDevice(e->device));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  ens_free(e);
  const size_t rows = (size_t)(n_worlds * n_bodies);
  std::vector<float> mass(rows);
  for (size_t i = 0; i < rows; ++i) mass[i] = weight ? (float)weight[i] : 1.0f;  // `weight as f32`, main.rs:360
  hipError_t h = hipMalloc((void**)&e->pos[0], rows * sizeof(float2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->pos[1], rows * sizeof(float2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->vel, rows * sizeof(float2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->mass, rows * sizeof(float));
  if (h == hipSuccess) h = hipMemcpyAsync(e->pos[0], pos, rows * sizeof(float2), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->vel, vel, rows * sizeof(float2), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->mass, mass.data(), rows * sizeof(float), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    ens_free(e);
    return ens_fail_hip(e, h, "upload");
  }
  e->n_worlds = n_worlds;
  e->n_bodies = n_bodies;
  return NBODY_OK;
}

NB_API int nbody_ensemble_download_f32(nbody_ensemble* e, float* pos, float* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, "ensemble download: nothing uploaded");
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_bodies) * sizeof(float2);
  if (pos) ENS_HIPCHK(e, hipMemcpyAsync(pos, e->pos[e->cur], bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) ENS_HIPCHK(e, hipMemcpyAsync(vel, e->vel, bytes, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

NB_API int64_t nbody_ensemble_num_worlds(const nbody_ensemble* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_ensemble_num_bodies(const nbody_ensemble* e) { return e ? e->n_bodies : 0; }

NB_API int nbody_ensemble_update_f32(nbody_ensemble* e, float delta, int n_steps, nbody_counting* counter) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, "ensemble update: nothing uploaded");
  if (n_steps < 0) return ens_fail(e, NBODY_ERR_INVALID, "ensemble update: n_steps < 0");
  if (n_steps == 0) return NBODY_OK;
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  for (int step = 0; step < n_steps; ++step) {
    EnsembleArgs a = ens_args(e);
    a.pos_out = e->pos[1 - e->cur];
    a.vel = e->vel;
    a.delta = delta;
    ENS_HIPCHK(e, launch_ensemble_step(e->stream, e->n_worlds, a));
    e->cur = 1 - e->cur;  // (the launches are in stream order: the next one reads what this one writes)
  }
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  // force and integration are one fused kernel: the whole call is booked under sum_gravity, as the direct step books it
  const double dt = now_s() - t_begin;
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
}

NB_API int nbody_ensemble_accel_f32(nbody_ensemble* e, float* acc_xy) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, "ensemble accel: nothing uploaded");
  if (!acc_xy) return ens_fail(e, NBODY_ERR_INVALID, "ensemble accel: acc_xy is NULL");
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_bodies) * sizeof(float2);
  if (!e->acc) ENS_HIPCHK(e, hipMalloc((void**)&e->acc, bytes));
  EnsembleArgs a = ens_args(e);
  a.acc_out = e->acc;
  ENS_HIPCHK(e, launch_ensemble_step(e->stream, e->n_worlds, a));
  ENS_HIPCHK(e, hipMemcpyAsync(acc_xy, e->acc, bytes, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}
