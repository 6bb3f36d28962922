// libnbody_hip — ensembles in f64: the handle and the C entry points of nbody_ensemble64_* (include/nbody_ensemble.h).  The
// sibling of ensemble.hip: the device probe and the stream are shared (ensemble_host.h); the rest is written out beside it
// rather than templated with it — element types, the masses kept as u32 weights, the arith rule and the kernel differ in every
// call, and the f32 exports stay what they were.  Many worlds of one size in world-major device arrays, every step of all of
// them one launch of ensemble64_kernels.hip on the handle's stream.  The positions are double-buffered across steps (a world's
// other blocks still read the old ones), velocities are updated in place.  No CPU path and no host synchronisation between the
// steps of a call.
#include <new>
#include <vector>

#include "driver.h"
#include "ensemble_host.h"
#include "ensemble64_kernels.h"

using namespace nbody;

struct nbody_ensemble64 {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  nbody_params params{};
  nbody_counting counting{};
  int64_t n_worlds = 0, n_bodies = 0;  // 0: nothing uploaded
  double2* pos[2] = {nullptr, nullptr};
  int cur = 0;
  double2* vel = nullptr;
  uint32_t* weight = nullptr;  // the kernel converts on use (`weight as f64` is exact)
  double2* acc = nullptr;
};

namespace {

thread_local std::string g_ens64_create_error;

int ens64_fail(nbody_ensemble64* e, int code, const std::string& msg) {
  if (e) e->err = msg; else g_ens64_create_error = msg;
  return code;
}
int ens64_fail_hip(nbody_ensemble64* e, hipError_t h, const char* what) {
  return ens64_fail(e, NBODY_ERR_HIP, std::string("ensemble: ") + what + ": " + hipGetErrorString(h));
}
#define ENS64_HIPCHK(e, call)                                   \
  do {                                                          \
    hipError_t h__ = (call);                                    \
    if (h__ != hipSuccess) return ens64_fail_hip(e, h__, #call); \
  } while (0)

void ens64_free(nbody_ensemble64* e) {
  free_dev(e->pos[0]); free_dev(e->pos[1]); free_dev(e->vel); free_dev(e->weight); free_dev(e->acc);
  e->n_worlds = e->n_bodies = 0;
  e->cur = 0;
}

Ensemble64Args ens64_args(const nbody_ensemble64* e) {
  Ensemble64Args a;
  a.pos_in = e->pos[e->cur];
  a.weight = e->weight;
  a.n_bodies = (int)e->n_bodies;
  a.clamp = (double)e->params.clamp;  // the f32 parameter widened, as the f64 context's direct step does
  a.fast = direct_fast_f64(e->params.arith, a.clamp) ? 1 : 0;  // opt-in, and a clamp that is not > 0 (or NaN): every world EXACT
  return a;
}

}  // namespace

NB_API int nbody_ensemble64_create(nbody_ensemble64** out, int device_id) {
  if (!out) return ens64_fail(nullptr, NBODY_ERR_INVALID, "nbody_ensemble64_create: out is NULL");
  *out = nullptr;
  hipStream_t stream = nullptr;
  std::string msg;
  const int rc = ensemble_open_device("nbody_ensemble64_create", device_id, &stream, msg);
  if (rc != NBODY_OK) return ens64_fail(nullptr, rc, msg);
  nbody_ensemble64* e = new (std::nothrow) nbody_ensemble64();
  if (!e) {
    ensemble_close_stream(stream);
    return ens64_fail(nullptr, NBODY_ERR_NOMEM, "nbody_ensemble64_create: out of host memory");
  }
  e->device = device_id;
  e->stream = stream;
  nbody_default_params(&e->params);
  *out = e;
  return NBODY_OK;
}

NB_API void nbody_ensemble64_destroy(nbody_ensemble64* e) {
  if (!e) return;
  ensemble_drain(e->device, e->stream);
  ens64_free(e);
  ensemble_close_stream(e->stream);
  delete e;
}

NB_API const char* nbody_ensemble64_last_error(const nbody_ensemble64* e) { return e ? e->err.c_str() : g_ens64_create_error.c_str(); }

NB_API int nbody_ensemble64_set_params(nbody_ensemble64* e, const nbody_params* p) {
  if (!e || !p) return NBODY_ERR_INVALID;
  if (p->arith < NBODY_ARITH_AUTO || p->arith > NBODY_ARITH_EXACT) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble set_params: bad arith");
  e->params = *p;
  return NBODY_OK;
}
NB_API int nbody_ensemble64_get_params(const nbody_ensemble64* e, nbody_params* out) {
  if (!e || !out) return NBODY_ERR_INVALID;
  *out = e->params;
  return NBODY_OK;
}

NB_API int nbody_ensemble64_upload(nbody_ensemble64* e, int64_t n_worlds, int64_t n_bodies, const double* pos, const double* vel,
                                   const uint32_t* weight) {
  if (!e) return NBODY_ERR_INVALID;
  if (n_bodies < 1 || n_bodies > kEnsembleMaxBodies)
    return ens64_fail(e, NBODY_ERR_INVALID, "ensemble upload: n_bodies must be 1 .. 4096 (above that a context per world is the tool)");
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows / n_bodies)
    return ens64_fail(e, NBODY_ERR_INVALID, "ensemble upload: n_worlds must be >= 1 and n_worlds * n_bodies <= 2^26");
  if (!pos || !vel) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble upload: pos_xy or vel_xy is NULL");
  ENS64_HIPCHK(e, hipSetDevice(e->device));
  ENS64_HIPCHK(e, hipStreamSynchronize(e->stream));
  ens64_free(e);
  const size_t rows = (size_t)(n_worlds * n_bodies);
  std::vector<uint32_t> ones;
  if (!weight) ones.assign(rows, 1u);
  const uint32_t* const w = weight ? weight : ones.data();
  hipError_t h = hipMalloc((void**)&e->pos[0], rows * sizeof(double2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->pos[1], rows * sizeof(double2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->vel, rows * sizeof(double2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->weight, rows * sizeof(uint32_t));
  if (h == hipSuccess) h = hipMemcpyAsync(e->pos[0], pos, rows * sizeof(double2), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->vel, vel, rows * sizeof(double2), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->weight, w, rows * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    ens64_free(e);
    return ens64_fail_hip(e, h, "upload");
  }
  e->n_worlds = n_worlds;
  e->n_bodies = n_bodies;
  return NBODY_OK;
}

NB_API int nbody_ensemble64_download(nbody_ensemble64* e, double* pos, double* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble download: nothing uploaded");
  ENS64_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_bodies) * sizeof(double2);
  if (pos) ENS64_HIPCHK(e, hipMemcpyAsync(pos, e->pos[e->cur], bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) ENS64_HIPCHK(e, hipMemcpyAsync(vel, e->vel, bytes, hipMemcpyDeviceToHost, e->stream));
  ENS64_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

NB_API int64_t nbody_ensemble64_num_worlds(const nbody_ensemble64* e) { return e ? e->n_worlds : 0; }
NB_API int64_t nbody_ensemble64_num_bodies(const nbody_ensemble64* e) { return e ? e->n_bodies : 0; }

NB_API int nbody_ensemble64_update(nbody_ensemble64* e, double delta, int n_steps, nbody_counting* counter) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble update: nothing uploaded");
  if (n_steps < 0) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble update: n_steps < 0");
  if (n_steps == 0) return NBODY_OK;
  ENS64_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  for (int step = 0; step < n_steps; ++step) {
    Ensemble64Args a = ens64_args(e);
    a.pos_out = e->pos[1 - e->cur];
    a.vel = e->vel;
    a.delta = delta;
    ENS64_HIPCHK(e, launch_ensemble64_step(e->stream, e->n_worlds, a));
    e->cur = 1 - e->cur;  // (the launches are in stream order: the next one reads what this one writes)
  }
  ENS64_HIPCHK(e, hipStreamSynchronize(e->stream));
  // force and integration are one fused kernel: the whole call is booked under sum_gravity, as the direct step books it
  const double dt = now_s() - t_begin;
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
}

NB_API int nbody_ensemble64_accel(nbody_ensemble64* e, double* acc_xy) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble accel: nothing uploaded");
  if (!acc_xy) return ens64_fail(e, NBODY_ERR_INVALID, "ensemble accel: acc_xy is NULL");
  ENS64_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_bodies) * sizeof(double2);
  if (!e->acc) ENS64_HIPCHK(e, hipMalloc((void**)&e->acc, bytes));
  Ensemble64Args a = ens64_args(e);
  a.acc_out = e->acc;
  ENS64_HIPCHK(e, launch_ensemble64_step(e->stream, e->n_worlds, a));
  ENS64_HIPCHK(e, hipMemcpyAsync(acc_xy, e->acc, bytes, hipMemcpyDeviceToHost, e->stream));
  ENS64_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}
