// libnbody_hip — ensembles: the host driver behind nbody_ensemble_* (ensemble.hip) and nbody_ensemble64_* (ensemble64.hip),
// written once over a precision P.  Internal.  Many worlds of one size in world-major device arrays, every step of all of them
// one launch on the handle's stream.  The positions are double-buffered across steps (a world's other blocks still read the
// old ones), velocities are updated in place.  No CPU path and no host synchronisation between the steps of a call.
//
// P supplies: Real, Vec2 (the element types), Mass (what the device keeps per body), Args (the kernel's arguments);
//   kCreate                        the create call's name, the prefix of its messages;
//   kWho                           the word that every other message of the handle begins with ("ensemble", "ragged", "restricted", "ragged restricted");
//   stage(weight, rows, tmp)       -> the rows Mass values to upload (tmp is theirs to fill);
//   route(args, mass, params)      the masses and the arithmetic of a launch, from the handle's parameters;
//   launch(stream, n_worlds, args) one step, or one force evaluation, of all worlds.
// A handle is a struct of its own derived from EnsembleState<P>: the C header declares distinct opaque types.
// The ragged handle (ragged_driver.h: worlds of different sizes, several launches per step) is built from the same parts: the
// state, create / destroy, params and errors as they are, and upload, download, update and accel through the *_rows / *_with
// functions below, which take the number of rows and the step's launches from their caller.
// The restricted handle (restricted_driver.h: tracers beside the bodies, a second launch per step) is the whole of this driver
// under its own kWho, with the tracers' launch added to a step through ens_update_with.
// Frames (nbody_frames_*, ensemble_frames.h) are ens_frames below for every handle: the ragged, restricted and ragged restricted
// drivers hand it their row ranges in a FrameRows and nothing else.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "driver.h"
#include "ensemble_frames.h"
#include "ensemble_kernels.h"

namespace nbody {

template <class P> struct EnsembleState {
  using Precision = P;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  nbody_params params{};
  nbody_counting counting{};
  int64_t n_worlds = 0, n_bodies = 0;  // 0: nothing uploaded (n_bodies stays 0 where the worlds have sizes of their own)
  int64_t rows = 0;                    // the rows of all worlds together
  typename P::Vec2* pos[2] = {nullptr, nullptr};
  int cur = 0;
  typename P::Vec2* vel = nullptr;
  typename P::Mass* mass = nullptr;
  typename P::Vec2* acc = nullptr;
  // frames (ens_frames): device scratch grown on demand, and a ragged handle's table of row ranges, uploaded by the first frames
  // call after an upload of bodies or tracers.  Freed with the arrays above.
  uint8_t* frame_rgba = nullptr;
  uint32_t* frame_work = nullptr;
  FrameWorld* frame_table = nullptr;
  size_t frame_rgba_bytes = 0, frame_work_bytes = 0;
  bool frame_table_valid = false;
};

template <class P> thread_local std::string g_ens_create_error;  // one per precision: what a failed create left for its thread

template <class P> int ens_fail(EnsembleState<P>* e, int code, const std::string& msg) {
  if (e) e->err = msg; else g_ens_create_error<P> = msg;
  return code;
}
template <class P> int ens_fail_hip(EnsembleState<P>* e, hipError_t h, const char* what) {
  return ens_fail<P>(e, NBODY_ERR_HIP, std::string(P::kWho) + ": " + what + ": " + hipGetErrorString(h));
}
#define ENS_HIPCHK(e, call)                                        \
  do {                                                             \
    hipError_t h__ = (call);                                       \
    if (h__ != hipSuccess) return ens_fail_hip<P>(e, h__, #call);  \
  } while (0)

template <class P> void ens_free(EnsembleState<P>* e) {
  free_dev(e->pos[0]); free_dev(e->pos[1]); free_dev(e->vel); free_dev(e->mass); free_dev(e->acc);
  free_dev(e->frame_rgba); free_dev(e->frame_work); free_dev(e->frame_table);
  e->frame_rgba_bytes = e->frame_work_bytes = 0;
  e->frame_table_valid = false;
  e->n_worlds = e->n_bodies = e->rows = 0;
  e->cur = 0;
}

template <class P> typename P::Args ens_args(const EnsembleState<P>* e) {
  typename P::Args a;
  a.pos_in = e->pos[e->cur];
  a.n_bodies = (int)e->n_bodies;
  P::route(a, e->mass, e->params);
  return a;
}

// Checks that device_id is a gfx950, makes it current, creates the handle's stream and then the handle H.
template <class H> int ens_create(H** out, int device_id) {
  using P = typename H::Precision;
  const std::string who = P::kCreate;
  if (!out) return ens_fail<P>(nullptr, NBODY_ERR_INVALID, who + ": out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t h = hipGetDeviceCount(&count);
  if (h != hipSuccess || count <= 0)
    return ens_fail<P>(nullptr, NBODY_ERR_NO_DEVICE,
                       who + ": no HIP device (" + (h != hipSuccess ? hipGetErrorString(h) : "count 0") + "); this library has no CPU path");
  if (device_id < 0 || device_id >= count) return ens_fail<P>(nullptr, NBODY_ERR_INVALID, who + ": device_id out of range");
  hipDeviceProp_t prop;
  h = hipGetDeviceProperties(&prop, device_id);
  if (h != hipSuccess) return ens_fail_hip<P>(nullptr, h, "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return ens_fail<P>(nullptr, NBODY_ERR_NO_DEVICE, who + ": device is " + prop.gcnArchName + ", kernels are built for gfx950 (MI355X) only");
  hipStream_t stream = nullptr;
  h = hipSetDevice(device_id);
  if (h == hipSuccess) h = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
  if (h != hipSuccess) return ens_fail_hip<P>(nullptr, h, P::kCreate);
  H* e = new (std::nothrow) H();
  if (!e) {
    (void)hipStreamDestroy(stream);
    return ens_fail<P>(nullptr, NBODY_ERR_NOMEM, who + ": out of host memory");
  }
  e->device = device_id;
  e->stream = stream;
  nbody_default_params(&e->params);
  *out = e;
  return NBODY_OK;
}

// The handle's device current and its stream drained before its buffers are freed.
template <class H> void ens_destroy(H* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  ens_free(e);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

template <class P> const char* ens_last_error(const EnsembleState<P>* e) { return e ? e->err.c_str() : g_ens_create_error<P>.c_str(); }

template <class P> int ens_set_params(EnsembleState<P>* e, const nbody_params* p) {
  if (!e || !p) return NBODY_ERR_INVALID;
  if (p->arith < NBODY_ARITH_AUTO || p->arith > NBODY_ARITH_EXACT) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " set_params: bad arith");
  e->params = *p;
  return NBODY_OK;
}
template <class P> int ens_get_params(const EnsembleState<P>* e, nbody_params* out) {
  if (!e || !out) return NBODY_ERR_INVALID;
  *out = e->params;
  return NBODY_OK;
}

// The handle's previous arrays freed and `rows` rows allocated and filled from the caller's (the stream is drained before and
// after).  On failure nothing is left allocated.
template <class P>
int ens_store_rows(EnsembleState<P>* e, int64_t n_rows, const typename P::Real* pos, const typename P::Real* vel, const uint32_t* weight) {
  using Vec2 = typename P::Vec2;
  using Mass = typename P::Mass;
  ENS_HIPCHK(e, hipSetDevice(e->device));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  ens_free(e);
  const size_t rows = (size_t)n_rows;
  std::vector<Mass> tmp;
  const Mass* const mass = P::stage(weight, rows, tmp);
  hipError_t h = hipMalloc((void**)&e->pos[0], rows * sizeof(Vec2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->pos[1], rows * sizeof(Vec2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->vel, rows * sizeof(Vec2));
  if (h == hipSuccess) h = hipMalloc((void**)&e->mass, rows * sizeof(Mass));
  if (h == hipSuccess) h = hipMemcpyAsync(e->pos[0], pos, rows * sizeof(Vec2), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->vel, vel, rows * sizeof(Vec2), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->mass, mass, rows * sizeof(Mass), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    ens_free(e);
    return ens_fail_hip(e, h, "upload");
  }
  e->rows = n_rows;
  return NBODY_OK;
}

// What an upload of worlds of one size refuses, before the handle is touched.
template <class P>
int ens_upload_check(EnsembleState<P>* e, int64_t n_worlds, int64_t n_bodies, const typename P::Real* pos, const typename P::Real* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (n_bodies < 1 || n_bodies > kEnsembleMaxBodies)
    return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " upload: n_bodies must be 1 .. 4096 (above that a context per world is the tool)");
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows / n_bodies)
    return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " upload: n_worlds must be >= 1 and n_worlds * n_bodies <= 2^26");
  if (!pos || !vel) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " upload: pos_xy or vel_xy is NULL");
  return NBODY_OK;
}

// The checked arguments stored as the handle's worlds.
template <class P>
int ens_upload_store(EnsembleState<P>* e, int64_t n_worlds, int64_t n_bodies, const typename P::Real* pos, const typename P::Real* vel,
                     const uint32_t* weight) {
  if (int rc = ens_store_rows(e, n_worlds * n_bodies, pos, vel, weight)) return rc;
  e->n_worlds = n_worlds;
  e->n_bodies = n_bodies;
  return NBODY_OK;
}

template <class P>
int ens_upload(EnsembleState<P>* e, int64_t n_worlds, int64_t n_bodies, const typename P::Real* pos, const typename P::Real* vel,
               const uint32_t* weight) {
  if (int rc = ens_upload_check(e, n_worlds, n_bodies, pos, vel)) return rc;
  return ens_upload_store(e, n_worlds, n_bodies, pos, vel, weight);
}

template <class P> int ens_download(EnsembleState<P>* e, typename P::Real* pos, typename P::Real* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " download: nothing uploaded");
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)e->rows * sizeof(typename P::Vec2);
  if (pos) ENS_HIPCHK(e, hipMemcpyAsync(pos, e->pos[e->cur], bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) ENS_HIPCHK(e, hipMemcpyAsync(vel, e->vel, bytes, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// n_steps steps; `launch(args)` enqueues one step (or one force evaluation) of every world on e->stream and returns a hipError_t.
template <class P, class Launch>
int ens_update_with(EnsembleState<P>* e, typename P::Real delta, int n_steps, nbody_counting* counter, Launch launch) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " update: nothing uploaded");
  if (n_steps < 0) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " update: n_steps < 0");
  if (n_steps == 0) return NBODY_OK;
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  for (int step = 0; step < n_steps; ++step) {
    typename P::Args a = ens_args(e);
    a.pos_out = e->pos[1 - e->cur];
    a.vel = e->vel;
    a.delta = delta;
    ENS_HIPCHK(e, launch(a));
    e->cur = 1 - e->cur;  // (the launches are in stream order: the next one reads what this one writes)
  }
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  // force and integration are one fused kernel: the whole call is booked under sum_gravity, as the direct step books it
  const double dt = now_s() - t_begin;
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
}

template <class P> int ens_update(EnsembleState<P>* e, typename P::Real delta, int n_steps, nbody_counting* counter) {
  return ens_update_with(e, delta, n_steps, counter, [e](const typename P::Args& a) { return P::launch(e->stream, e->n_worlds, a); });
}

template <class P, class Launch> int ens_accel_with(EnsembleState<P>* e, typename P::Real* acc_xy, Launch launch) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " accel: nothing uploaded");
  if (!acc_xy) return ens_fail(e, NBODY_ERR_INVALID, std::string(P::kWho) + " accel: acc_xy is NULL");
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)e->rows * sizeof(typename P::Vec2);
  if (!e->acc) ENS_HIPCHK(e, hipMalloc((void**)&e->acc, bytes));
  typename P::Args a = ens_args(e);
  a.acc_out = e->acc;
  ENS_HIPCHK(e, launch(a));
  ENS_HIPCHK(e, hipMemcpyAsync(acc_xy, e->acc, bytes, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

template <class P> int ens_accel(EnsembleState<P>* e, typename P::Real* acc_xy) {
  return ens_accel_with(e, acc_xy, [e](const typename P::Args& a) { return P::launch(e->stream, e->n_worlds, a); });
}

// ---- frames: every world's draw() raster (ensemble_frames.h) of the current positions, into host memory
// What a handle tells ens_frames about its rows, beyond the bodies of worlds of one size.
template <class P> struct FrameRows {
  const int64_t* sizes = nullptr;         // worlds of different sizes: the bodies per world; NULL: e->n_bodies in every world
  const int64_t* counts = nullptr;        // with sizes: the tracers per world, or NULL: none (kept whether or not they are painted)
  int64_t n_tracers = 0;                  // without sizes: the tracers per world
  const typename P::Vec2* tpos = nullptr; // the tracers to paint after the bodies, or NULL: the bodies' frames
  const typename P::Vec2* tvel = nullptr;
};

// A device buffer of at least `need` bytes; a smaller one is freed and replaced.
template <class P, class B> int ens_frame_buffer(EnsembleState<P>* e, B*& p, size_t& bytes, size_t need) {
  if (bytes >= need) return NBODY_OK;
  free_dev(p);
  bytes = 0;
  ENS_HIPCHK(e, hipMalloc((void**)&p, need));
  bytes = need;
  return NBODY_OK;
}

// rgba_out: [n_worlds][render_px][render_px][4] bytes.  Synchronous, on the handle's stream; reads pos[cur], writes no state.
// Every refusal comes before anything is allocated or launched.
template <class P>
int ens_frames(EnsembleState<P>* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out, const FrameRows<P>& rows = FrameRows<P>()) {
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " frames: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!rgba_out) return ens_fail(e, NBODY_ERR_INVALID, who + "rgba_out is NULL");
  // main.rs:51-52 divide by HEIGHT / RENDER_HEIGHT: a cell of 0 world units or a last cell past the frame is an out-of-range
  // index upstream (a panic): refused, as nbody_render_rgba refuses it
  if (height == 0 || render_px == 0) return ens_fail(e, NBODY_ERR_INVALID, who + "height and render_px must be > 0");
  if (height % render_px != 0 || height > kFrameMaxHeight)
    return ens_fail(e, NBODY_ERR_INVALID, who + "render_px must divide height (height <= 2^24)");
  const int64_t npix = (int64_t)render_px * render_px;  // <= 2^48
  if (e->n_worlds > kFrameMaxPixels / npix) return ens_fail(e, NBODY_ERR_INVALID, who + "n_worlds * render_px^2 must be <= 2^26 pixels");
  const bool tracers = rows.tpos != nullptr;
  int64_t max_rows = e->n_bodies + (tracers ? rows.n_tracers : 0);
  if (rows.sizes)
    for (int64_t k = 0; k < e->n_worlds; ++k) max_rows = std::max(max_rows, rows.sizes[k] + (tracers && rows.counts ? rows.counts[k] : 0));
  // (a world has at most 4096 bodies: only the sum with its tracers can pass 2^24)
  if (max_rows > kFrameMaxRows)
    return ens_fail(e, NBODY_ERR_INVALID, who + "a world's bodies and tracers together must be <= 2^24 rows (paint it without tracers)");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const bool lds = frame_route_lds(render_px);
  if (int rc = ens_frame_buffer(e, e->frame_rgba, e->frame_rgba_bytes, (size_t)(e->n_worlds * npix) * 4)) return rc;
  if (!lds)
    if (int rc = ens_frame_buffer(e, e->frame_work, e->frame_work_bytes, (size_t)(e->n_worlds * npix) * 2 * sizeof(uint32_t))) return rc;
  if (rows.sizes && !e->frame_table_valid) {
    std::vector<FrameWorld> table((size_t)e->n_worlds);
    int64_t row0 = 0, trow0 = 0;
    for (int64_t k = 0; k < e->n_worlds; ++k) {
      const int64_t m = rows.counts ? rows.counts[k] : 0;
      table[(size_t)k] = FrameWorld{(uint32_t)row0, (uint32_t)rows.sizes[k], (uint32_t)trow0, (uint32_t)m};  // (each sum <= 2^26)
      row0 += rows.sizes[k];
      trow0 += m;
    }
    if (!e->frame_table) ENS_HIPCHK(e, hipMalloc((void**)&e->frame_table, table.size() * sizeof(FrameWorld)));
    ENS_HIPCHK(e, hipMemcpyAsync(e->frame_table, table.data(), table.size() * sizeof(FrameWorld), hipMemcpyHostToDevice, e->stream));
    ENS_HIPCHK(e, hipStreamSynchronize(e->stream));  // (`table` goes out of scope)
    e->frame_table_valid = true;
  }
  FrameArgs a;
  a.pos = e->pos[e->cur];
  a.vel = e->vel;
  a.mass = e->mass;
  a.tpos = rows.tpos;
  a.tvel = rows.tvel;
  a.table = rows.sizes ? e->frame_table : nullptr;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = tracers ? (uint32_t)rows.n_tracers : 0u;
  a.height = height;
  a.render_px = render_px;
  ENS_HIPCHK(e, launch_ensemble_frames<typename P::Real>(e->stream, e->n_worlds, max_rows, a, lds ? nullptr : e->frame_work, e->frame_rgba));
  ENS_HIPCHK(e, hipMemcpyAsync(rgba_out, e->frame_rgba, (size_t)(e->n_worlds * npix) * 4, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

#undef ENS_HIPCHK

}  // namespace nbody
