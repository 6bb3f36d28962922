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
//   SweepWorld, sweep_world(delta, clamp, steps), sweep_route(args, params)
//                                  sweeps (ens_sweep_with): a world's entry of the kernels' table, and the call-wide arithmetic
//                                  where every world brings a clamp of its own (params.arith alone: the clamp's test is the kernels');
//   launch(stream, n_worlds, args) one step, or one force evaluation, of all worlds.
// A handle is a struct of its own derived from EnsembleState<P>: the C header declares distinct opaque types.
// The ragged handle (ragged_driver.h: worlds of different sizes, several launches per step) is built from the same parts: the
// state, create / destroy, params and errors as they are, and upload, download, update and accel through the *_rows / *_with
// functions below, which take the number of rows and the step's launches from their caller.
// The restricted handle (restricted_driver.h: tracers beside the bodies, a second launch per step) is the whole of this driver
// under its own kWho, with the tracers' launch added to a step through ens_update_with.
// Frames (nbody_frames_*, ensemble_frames.h) are ens_frames below for every handle: the ragged, restricted and ragged restricted
// drivers hand it their row ranges in a FrameRows and nothing else.
// Delta streams (nbody_deltas_*, ensemble_deltas.h) are ens_deltas below for every handle in the same way: the other drivers hand
// it their sizes, counts and tracer positions in a DeltaRows.  The state counts its steps (`updates`) for the streams' headers.
// Sweeps (nbody_sweep_*: a time step, a clamp and a number of steps per world) are ens_sweep_with below for every handle: the
// other drivers supply the launches of a step, as they do for ens_update_with.
// Summaries (nbody_summary_*, ensemble_summary.h) are ens_summary below for every handle: the other drivers hand it their sizes,
// counts and tracer arrays in a SummaryRows; a ragged handle's row ranges are the frames' table.
// Encounters (nbody_encounters_*, ensemble_encounters.h) are ens_encounters below for every handle in the same way, over an
// EncounterRows.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "driver.h"
#include "ensemble_deltas.h"
#include "ensemble_encounters.h"
#include "ensemble_frames.h"
#include "ensemble_kernels.h"
#include "ensemble_summary.h"

namespace nbody {

// One sequence of delta streams of a handle (ens_deltas): the bodies' or the tracers'.  Everything is device scratch of the
// handle, made by the first call after an upload of the rows it describes and freed where those rows are freed, which is also
// how an upload resets the sequence (the next streams are key frames).
struct DeltaSeq {
  bool planned = false;        // blocks and base_total below are those of the current rows
  bool ready = false;          // the scratch below is allocated for them
  int64_t blocks = 0;          // 64-row blocks of all segments together
  uint64_t base_total = 0;     // sum over the segments of (32 + width bytes)
  void* keys[3] = {nullptr, nullptr, nullptr};
  int cur = 0;                 // keys[cur] is written next; prev = keys[(cur + 2) % 3], prev2 = keys[(cur + 1) % 3]
  uint32_t have = 0;           // how many of prev, prev2 hold keys of this sequence (0: the next stream is a key frame)
  uint8_t* widths = nullptr;
  uint32_t* words = nullptr;
  uint32_t* offsets = nullptr;
  void* scan = nullptr;
  size_t scan_bytes = 0;
  DeltaSeg* table = nullptr;   // ragged handles
  uint32_t* seg_of_block = nullptr;
  uint64_t* stream_off = nullptr;
  uint8_t* out = nullptr;      // grown to the streams of a call
  size_t out_bytes = 0;
  void release() {
    for (auto& k : keys) free_dev(k);
    free_dev(widths); free_dev(words); free_dev(offsets); free_dev(scan); free_dev(table); free_dev(seg_of_block);
    free_dev(stream_off); free_dev(out);
    *this = DeltaSeq();
  }
};

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
  // delta streams (ens_deltas): the steps taken since the handle was created (it runs on across uploads, as a context's count
  // does), and the two sequences.  The bodies' goes with the arrays above; the tracers' with the tracers of the handles that
  // have them (and so with the bodies too: an upload of bodies removes the tracers).
  uint64_t updates = 0;
  DeltaSeq dbodies, dtracers;
  // sweeps (ens_sweep_with): the table of the worlds' entries of the call in flight, on the host and on the device.  Scratch:
  // grown on demand, rewritten by every call, nothing of a sweep outlives it.  Freed with the arrays above.
  std::vector<typename P::SweepWorld> sweep_host;
  typename P::SweepWorld* sweep_dev = nullptr;
  size_t sweep_dev_bytes = 0;
  // summaries (ens_summary): the records, the chunk records of segments of several chunks and the call's ref[], all device
  // scratch grown on demand; beside the frames' table (and valid with it) the first chunk of every world's tracers, for a ragged
  // handle.  Freed with the arrays above.
  nbody_world_summary* summary_out = nullptr;
  nbody_world_summary* summary_chunks = nullptr;
  int32_t* summary_ref = nullptr;
  size_t summary_out_bytes = 0, summary_chunks_bytes = 0, summary_ref_bytes = 0;
  uint32_t* summary_chunk_base = nullptr;
  int64_t summary_tracer_chunks = 0;
  // encounters (ens_encounters): the records, the four per-target arrays and the call's limit2[], all device scratch grown on
  // demand; beside the frames' table (and valid with it) the first tile of every world's bodies and of its tracers, for a ragged
  // handle.  Freed with the arrays above.
  nbody_world_encounters* enc_out = nullptr;
  int32_t* enc_index = nullptr;
  void* enc_d2 = nullptr;
  uint32_t* enc_close = nullptr;
  uint32_t* enc_live = nullptr;
  float* enc_limit = nullptr;
  size_t enc_out_bytes = 0, enc_index_bytes = 0, enc_d2_bytes = 0, enc_close_bytes = 0, enc_live_bytes = 0, enc_limit_bytes = 0;
  uint32_t* enc_tile_base = nullptr;  // [2][n_worlds + 1]: the bodies', then the tracers'
  int64_t enc_body_tiles = 0, enc_tracer_tiles = 0;
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
  free_dev(e->sweep_dev);
  e->sweep_dev_bytes = 0;
  free_dev(e->summary_out); free_dev(e->summary_chunks); free_dev(e->summary_ref); free_dev(e->summary_chunk_base);
  e->summary_out_bytes = e->summary_chunks_bytes = e->summary_ref_bytes = 0;
  e->summary_tracer_chunks = 0;
  free_dev(e->enc_out); free_dev(e->enc_index); free_dev(e->enc_d2); free_dev(e->enc_close); free_dev(e->enc_live); free_dev(e->enc_limit);
  free_dev(e->enc_tile_base);
  e->enc_out_bytes = e->enc_index_bytes = e->enc_d2_bytes = e->enc_close_bytes = e->enc_live_bytes = e->enc_limit_bytes = 0;
  e->enc_body_tiles = e->enc_tracer_tiles = 0;
  e->dbodies.release();
  e->dtracers.release();
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

template <class P, class B> int ens_frame_buffer(EnsembleState<P>* e, B*& p, size_t& bytes, size_t need);  // (below: a grown device buffer)

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
    ++e->updates;
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

// A sweep: n_steps steps in which world k steps by delta[k] under clamp[k] (NULL: params.clamp in every world) and takes the
// first steps[k] of them (NULL: all), then stands still; `launch(args)` as in ens_update_with.  Every refusal comes before
// anything is allocated or enqueued.  The three arrays are read here, into the table the kernels read: the call keeps nothing.
// Every launch steps the handle's count and flips the position buffers for all worlds, finished or not: a finished world's
// blocks carry its positions over (ensemble_kernels.hip, "Sweeps").
template <class P, class Launch>
int ens_sweep_with(EnsembleState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps,
                   nbody_counting* counter, Launch launch) {
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " sweep: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!delta) return ens_fail(e, NBODY_ERR_INVALID, who + "delta is NULL");
  if (n_steps < 0) return ens_fail(e, NBODY_ERR_INVALID, who + "n_steps < 0");
  if (steps)
    for (int64_t k = 0; k < e->n_worlds; ++k)
      if (steps[k] < 0 || steps[k] > n_steps)
        return ens_fail(e, NBODY_ERR_INVALID, who + "steps[" + std::to_string(k) + "] = " + std::to_string(steps[k]) + " of world " +
                                                  std::to_string(k) + " is outside 0 .. n_steps = " + std::to_string(n_steps));
  if (n_steps == 0) return NBODY_OK;
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  const size_t n = (size_t)e->n_worlds, bytes = n * sizeof(typename P::SweepWorld);
  e->sweep_host.resize(n);  // (the handle's: the copy below may still read it when an error returns early)
  for (size_t k = 0; k < n; ++k) e->sweep_host[k] = P::sweep_world(delta[k], clamp ? clamp[k] : e->params.clamp, steps ? steps[k] : n_steps);
  if (int rc = ens_frame_buffer(e, e->sweep_dev, e->sweep_dev_bytes, bytes)) return rc;
  ENS_HIPCHK(e, hipMemcpyAsync(e->sweep_dev, e->sweep_host.data(), bytes, hipMemcpyHostToDevice, e->stream));
  for (int step = 0; step < n_steps; ++step) {
    typename P::Args a = ens_args(e);
    if (clamp) P::sweep_route(a, e->params);
    a.pos_out = e->pos[1 - e->cur];
    a.vel = e->vel;
    a.sweep = e->sweep_dev;
    a.step = step;
    ENS_HIPCHK(e, launch(a));
    e->cur = 1 - e->cur;
    ++e->updates;
  }
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  const double dt = now_s() - t_begin;  // booked as an update's seconds are
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
}

template <class P>
int ens_sweep(EnsembleState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter) {
  return ens_sweep_with(e, delta, clamp, steps, n_steps, counter,
                        [e](const typename P::Args& a) { return P::launch(e->stream, e->n_worlds, a); });
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

// A ragged handle's table of row ranges on the device (sizes: the bodies per world; counts: the tracers per world, or NULL: none),
// uploaded by the first frames, summary or encounters call after an upload of bodies or tracers.  Beside it, for the summaries,
// the first chunk of every world's tracers among the chunks of all worlds' tracers, and their total; for the encounters, the first
// tile of every world's bodies among the tiles of all worlds' bodies, the same for the tracers, and the two totals.
template <class P> int ens_frame_table(EnsembleState<P>* e, const int64_t* sizes, const int64_t* counts) {
  if (e->frame_table_valid) return NBODY_OK;
  const size_t n = (size_t)e->n_worlds;
  std::vector<FrameWorld> table(n);
  std::vector<uint32_t> chunk_base(n + 1), tile_base(2 * (n + 1));
  int64_t row0 = 0, trow0 = 0, chunk0 = 0, tile0 = 0, ttile0 = 0;
  for (size_t k = 0; k < n; ++k) {
    const int64_t m = counts ? counts[k] : 0;
    table[k] = FrameWorld{(uint32_t)row0, (uint32_t)sizes[k], (uint32_t)trow0, (uint32_t)m};  // (each sum <= 2^26)
    chunk_base[k] = (uint32_t)chunk0;                                                          // (<= 2^26 worlds + 2^14 full chunks)
    row0 += sizes[k];
    trow0 += m;
    chunk0 += summary_chunks((uint32_t)m);
    tile_base[k] = (uint32_t)tile0;                                                            // (<= 2^26 worlds + 2^18 full tiles)
    tile_base[n + 1 + k] = (uint32_t)ttile0;
    tile0 += encounter_tiles((uint32_t)sizes[k]);
    ttile0 += encounter_tiles((uint32_t)m);
  }
  chunk_base[n] = (uint32_t)chunk0;
  tile_base[n] = (uint32_t)tile0;
  tile_base[2 * n + 1] = (uint32_t)ttile0;
  if (!e->frame_table) ENS_HIPCHK(e, hipMalloc((void**)&e->frame_table, n * sizeof(FrameWorld)));
  if (!e->summary_chunk_base) ENS_HIPCHK(e, hipMalloc((void**)&e->summary_chunk_base, (n + 1) * sizeof(uint32_t)));
  ENS_HIPCHK(e, hipMemcpyAsync(e->frame_table, table.data(), n * sizeof(FrameWorld), hipMemcpyHostToDevice, e->stream));
  if (!e->enc_tile_base) ENS_HIPCHK(e, hipMalloc((void**)&e->enc_tile_base, 2 * (n + 1) * sizeof(uint32_t)));
  ENS_HIPCHK(e, hipMemcpyAsync(e->summary_chunk_base, chunk_base.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  ENS_HIPCHK(e, hipMemcpyAsync(e->enc_tile_base, tile_base.data(), 2 * (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));  // (the vectors go out of scope)
  e->summary_tracer_chunks = chunk0;
  e->enc_body_tiles = tile0;
  e->enc_tracer_tiles = ttile0;
  e->frame_table_valid = true;
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
  if (rows.sizes)
    if (int rc = ens_frame_table(e, rows.sizes, rows.counts)) return rc;
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

// ---- delta streams: every world's NBD1 stream (ensemble_deltas.h) of the current positions, into host memory
// What a handle tells ens_deltas about its rows, beyond the bodies of worlds of one size.
template <class P> struct DeltaRows {
  const int64_t* sizes = nullptr;         // worlds of different sizes: the bodies per world; NULL: e->n_bodies in every world
  const int64_t* counts = nullptr;        // with sizes: the tracers per world, or NULL: none
  int64_t n_tracers = 0;                  // without sizes: the tracers per world
  const typename P::Vec2* tpos = nullptr; // the tracers' positions (NULL where the handle holds none)
  bool tracer_calls = false;              // the handle has tracer calls at all: NBODY_DELTAS_TRACERS is its to ask
};

// The scratch of a sequence for its planned rows; on failure the sequence is released whole.
template <class P> int ens_deltas_scratch(EnsembleState<P>* e, DeltaSeq& q, bool tracers, const DeltaRows<P>& rows) {
  const size_t blocks = (size_t)q.blocks, kb = blocks * 128 * sizeof(typename P::Real);
  q.scan_bytes = deltas_scan_temp_bytes(q.blocks);
  hipError_t h = hipSuccess;
  for (auto& k : q.keys)
    if (h == hipSuccess) h = hipMalloc(&k, kb ? kb : 8);
  if (h == hipSuccess) h = hipMalloc((void**)&q.widths, 2 * blocks + 8);
  if (h == hipSuccess) h = hipMalloc((void**)&q.words, (2 * blocks + 1) * 4);
  if (h == hipSuccess) h = hipMalloc((void**)&q.offsets, (2 * blocks + 1) * 4);
  if (h == hipSuccess) h = hipMalloc(&q.scan, q.scan_bytes ? q.scan_bytes : 8);
  if (h == hipSuccess) h = hipMalloc((void**)&q.stream_off, ((size_t)e->n_worlds + 1) * 8);
  if (h == hipSuccess) h = hipMemsetAsync(q.words, 0, (2 * blocks + 1) * 4, e->stream);    // (the scan reads the last entry too)
  if (h == hipSuccess) h = hipMemsetAsync(q.offsets, 0, (2 * blocks + 1) * 4, e->stream);  // (without a block it is never written)
  if (h == hipSuccess && rows.sizes) {  // the table of a ragged handle: built here, once per upload of the rows it describes
    std::vector<DeltaSeg> table((size_t)e->n_worlds);
    std::vector<uint32_t> seg_of_block(blocks);
    uint64_t row0 = 0, blk0 = 0, base = 0;
    for (int64_t k = 0; k < e->n_worlds; ++k) {
      const int64_t n = tracers ? (rows.counts ? rows.counts[k] : 0) : rows.sizes[k];
      table[(size_t)k] = DeltaSeg{(uint32_t)row0, (uint32_t)n, (uint32_t)blk0, 0u, base};  // (rows <= 2^26, blocks <= 2^24)
      for (size_t b = 0; b < delta_blocks(n); ++b) seg_of_block[blk0 + b] = (uint32_t)k;
      row0 += (uint64_t)n;
      blk0 += delta_blocks(n);
      base += kDeltaHeader + delta_width_bytes(n);
    }
    h = hipMalloc((void**)&q.table, table.size() * sizeof(DeltaSeg));
    if (h == hipSuccess) h = hipMalloc((void**)&q.seg_of_block, blocks ? blocks * 4 : 8);
    if (h == hipSuccess) h = hipMemcpyAsync(q.table, table.data(), table.size() * sizeof(DeltaSeg), hipMemcpyHostToDevice, e->stream);
    if (h == hipSuccess && blocks) h = hipMemcpyAsync(q.seg_of_block, seg_of_block.data(), blocks * 4, hipMemcpyHostToDevice, e->stream);
    if (h == hipSuccess) h = hipStreamSynchronize(e->stream);  // (the vectors go out of scope)
  }
  if (h != hipSuccess) {
    (void)hipStreamSynchronize(e->stream);
    q.release();
    return ens_fail_hip(e, h, "the scratch of the delta streams");
  }
  q.ready = true;
  return NBODY_OK;
}

// One stream per world, one after another in world order, into out[0, cap); offsets_out (may be NULL): [n_worlds + 1].
// Synchronous, on the handle's stream; reads pos[cur] or the tracers, writes no simulation state.  The sequence advances only
// when the streams have been copied out: a refused call changes nothing.
template <class P>
int ens_deltas(EnsembleState<P>* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out, uint64_t* step_out,
               const DeltaRows<P>& rows = DeltaRows<P>()) {
  using K = typename std::conditional<sizeof(typename P::Real) == 8, uint64_t, uint32_t>::type;
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " deltas: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!bytes_out) return ens_fail(e, NBODY_ERR_INVALID, who + "bytes_out is NULL");
  if (!out && cap) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL with cap != 0");
  if (flags & ~(NBODY_DELTAS_TRACERS | NBODY_DELTAS_KEY)) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_DELTAS_TRACERS) != 0;
  if (tracers && !rows.tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_DELTAS_TRACERS on a handle without tracers");
  DeltaSeq& q = tracers ? e->dtracers : e->dbodies;
  if (!q.planned) {  // (once per upload of these rows: the only loop over worlds, and only for a ragged handle)
    int64_t blocks = 0;
    uint64_t base = 0;
    if (rows.sizes) {
      for (int64_t k = 0; k < e->n_worlds; ++k) {
        const int64_t n = tracers ? (rows.counts ? rows.counts[k] : 0) : rows.sizes[k];
        blocks += (int64_t)delta_blocks(n);
        base += kDeltaHeader + delta_width_bytes(n);
      }
    } else {
      const int64_t n = tracers ? rows.n_tracers : e->n_bodies;
      blocks = e->n_worlds * (int64_t)delta_blocks(n);  // (rows <= 2^26)
      base = (uint64_t)e->n_worlds * (kDeltaHeader + delta_width_bytes(n));
    }
    q.blocks = blocks;
    q.base_total = base;
    q.planned = true;
  }
  if (q.blocks > kDeltasMaxBlocks)
    return ens_fail(e, NBODY_ERR_INVALID, who + "more than 2^24 blocks of 64 rows in the worlds together (nbody_deltas_bound)");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  if (!q.ready)
    if (int rc = ens_deltas_scratch(e, q, tracers, rows)) return rc;
  DeltasArgs a;
  a.pos = tracers ? (const void*)rows.tpos : (const void*)e->pos[e->cur];
  a.table = q.table;
  a.seg_of_block = q.seg_of_block;
  a.n_segs = (uint32_t)e->n_worlds;
  a.n = rows.sizes ? 0u : (uint32_t)(tracers ? rows.n_tracers : e->n_bodies);
  a.blocks = (uint32_t)q.blocks;
  a.have = (flags & NBODY_DELTAS_KEY) ? 0u : q.have;
  a.step = e->updates;
  a.base_total = q.base_total;
  a.cur = q.keys[q.cur];
  a.prev = q.keys[(q.cur + 2) % 3];
  a.prev2 = q.keys[(q.cur + 1) % 3];
  a.widths = q.widths;
  a.words = q.words;
  a.offsets = q.offsets;
  a.stream_off = q.stream_off;
  // the size of the streams is known on the device only: measure, fetch it, then write the streams at their final places
  uint32_t words = 0;
  if (q.blocks) {
    ENS_HIPCHK(e, launch_deltas_measure<K>(e->stream, a, q.scan, q.scan_bytes));
    ENS_HIPCHK(e, hipMemcpyAsync(&words, q.offsets + 2 * q.blocks, 4, hipMemcpyDeviceToHost, e->stream));
    ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
    if ((uint64_t)words > 2 * (uint64_t)q.blocks * sizeof(K) * 8) return ens_fail(e, NBODY_ERR_HIP, who + "the encoder reported an impossible size");
  }
  const size_t total = (size_t)q.base_total + (size_t)words * 8;
  *bytes_out = total;
  if (!out || cap < total) return ens_fail(e, NBODY_ERR_INVALID, who + "the output buffer is smaller than the stream");
  if (int rc = ens_frame_buffer(e, q.out, q.out_bytes, total)) return rc;
  a.out = q.out;
  ENS_HIPCHK(e, launch_deltas_write<K>(e->stream, a));
  ENS_HIPCHK(e, hipMemcpyAsync(out, q.out, total, hipMemcpyDeviceToHost, e->stream));
  if (offsets_out)
    ENS_HIPCHK(e, hipMemcpyAsync(offsets_out, q.stream_off, ((size_t)e->n_worlds + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  if (step_out) *step_out = e->updates;
  q.cur = (q.cur + 1) % 3;  // the oldest keys are overwritten next time
  q.have = a.have < 2 ? a.have + 1 : 2;
  return NBODY_OK;
}

// ---- summaries: one nbody_world_summary per world (ensemble_summary.h) of the current rows, into host memory
// What a handle tells ens_summary about its rows, beyond the bodies of worlds of one size.
template <class P> struct SummaryRows {
  const int64_t* sizes = nullptr;         // worlds of different sizes: the bodies per world; NULL: e->n_bodies in every world
  const int64_t* counts = nullptr;        // with sizes: the tracers per world, or NULL: none
  int64_t n_tracers = 0;                  // without sizes: the tracers per world
  const typename P::Vec2* tpos = nullptr; // the tracers (NULL where the handle holds none)
  const typename P::Vec2* tvel = nullptr;
  bool tracer_calls = false;              // the handle has tracer calls at all: NBODY_SUMMARY_TRACERS is its to ask
};

// out: [n_worlds] records.  Synchronous, on the handle's stream; reads pos[cur], vel, the masses or the tracers, writes no state.
// Every refusal comes before anything is allocated or launched.  One launch for the bodies, two for the tracers where a world
// has more than 4096 of them; the only loops over worlds are the check of ref[] and, once per upload, a ragged handle's table.
template <class P>
int ens_summary(EnsembleState<P>* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out,
                const SummaryRows<P>& rows = SummaryRows<P>()) {
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " summary: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!out) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL");
  if (flags & ~NBODY_SUMMARY_TRACERS) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_SUMMARY_TRACERS) != 0;
  if (tracers && !rows.tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_SUMMARY_TRACERS on a handle without tracers");
  if (height > kSummaryMaxHeight) return ens_fail(e, NBODY_ERR_INVALID, who + "height must be <= 2^24");
  const auto seg_rows = [&](int64_t k) { return tracers ? (rows.counts ? rows.counts[k] : 0) : rows.sizes[k]; };  // (ragged handles)
  if (ref)
    for (int64_t k = 0; k < e->n_worlds; ++k) {
      const int64_t j = ref[k];
      if (j >= -1 && j < e->n_worlds && !(rows.sizes && j >= 0 && seg_rows(j) != seg_rows(k))) continue;
      const std::string which = "ref[" + std::to_string(k) + "] = " + std::to_string(j) + " of world " + std::to_string(k);
      if (j < -1 || j >= e->n_worlds)
        return ens_fail(e, NBODY_ERR_INVALID, who + which + " is outside -1 .. n_worlds - 1 = " + std::to_string(e->n_worlds - 1));
      return ens_fail(e, NBODY_ERR_INVALID, who + which + " names a world of " + std::to_string(seg_rows(j)) + " rows, world " +
                                                  std::to_string(k) + " has " + std::to_string(seg_rows(k)));
    }

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t n = (size_t)e->n_worlds;
  int64_t n_chunks = e->n_worlds;
  if (rows.sizes) {
    if (int rc = ens_frame_table(e, rows.sizes, rows.counts)) return rc;
    if (tracers) n_chunks = e->summary_tracer_chunks;
  } else {
    n_chunks = e->n_worlds * (int64_t)summary_chunks((uint32_t)(tracers ? rows.n_tracers : e->n_bodies));
  }
  if (int rc = ens_frame_buffer(e, e->summary_out, e->summary_out_bytes, n * sizeof(nbody_world_summary))) return rc;
  if (n_chunks > e->n_worlds)
    if (int rc = ens_frame_buffer(e, e->summary_chunks, e->summary_chunks_bytes, (size_t)n_chunks * sizeof(nbody_world_summary))) return rc;
  if (ref) {
    if (int rc = ens_frame_buffer(e, e->summary_ref, e->summary_ref_bytes, n * sizeof(int32_t))) return rc;
    ENS_HIPCHK(e, hipMemcpyAsync(e->summary_ref, ref, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  }
  SummaryArgs a;
  a.pos = e->pos[e->cur];
  a.vel = e->vel;
  a.mass = e->mass;
  a.tpos = rows.tpos;
  a.tvel = rows.tvel;
  a.table = rows.sizes ? e->frame_table : nullptr;
  a.chunk_base = rows.sizes ? e->summary_chunk_base : nullptr;
  a.ref = ref ? e->summary_ref : nullptr;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = (uint32_t)rows.n_tracers;
  a.n_worlds = (uint32_t)e->n_worlds;
  a.height = height;
  a.tracers = tracers ? 1u : 0u;
  ENS_HIPCHK(e, launch_ensemble_summary<typename P::Real>(e->stream, a, n_chunks, e->summary_chunks, e->summary_out));
  ENS_HIPCHK(e, hipMemcpyAsync(out, e->summary_out, n * sizeof(nbody_world_summary), hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// ---- encounters: per target its nearest source and its clamped pairs, per world one nbody_world_encounters
// (ensemble_encounters.h) of the current rows, into host memory
// What a handle tells ens_encounters about its rows, beyond the bodies of worlds of one size.
template <class P> struct EncounterRows {
  const int64_t* sizes = nullptr;         // worlds of different sizes: the bodies per world; NULL: e->n_bodies in every world
  const int64_t* counts = nullptr;        // with sizes: the tracers per world, or NULL: none
  int64_t n_tracers = 0;                  // without sizes: the tracers per world
  int64_t tracer_rows = 0;                // with sizes: the tracers of all worlds together
  const typename P::Vec2* tpos = nullptr; // the tracers (NULL where the handle holds none)
  bool tracer_calls = false;              // the handle has tracer calls at all: NBODY_ENCOUNTERS_TRACERS is its to ask
};

// out: [n_worlds] records; nn_index, nn_d2, close: one entry per target of all worlds, each may be NULL.  Synchronous, on the
// handle's stream; reads pos[cur] and the tracers' positions, writes no state.  Every refusal comes before anything is allocated
// or launched.  Two launches; no loop over worlds but, once per upload, a ragged handle's table.
template <class P>
int ens_encounters(EnsembleState<P>* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index,
                   typename P::Real* nn_d2, uint32_t* close, const EncounterRows<P>& rows = EncounterRows<P>()) {
  using Real = typename P::Real;
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " encounters: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!out) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL");
  if (flags & ~NBODY_ENCOUNTERS_TRACERS) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_ENCOUNTERS_TRACERS) != 0;
  if (tracers && !rows.tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_ENCOUNTERS_TRACERS on a handle without tracers");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t n = (size_t)e->n_worlds;
  int64_t n_tiles, targets;
  if (rows.sizes) {
    if (int rc = ens_frame_table(e, rows.sizes, rows.counts)) return rc;
    n_tiles = tracers ? e->enc_tracer_tiles : e->enc_body_tiles;
    targets = tracers ? rows.tracer_rows : e->rows;
  } else {
    const int64_t per_world = tracers ? rows.n_tracers : e->n_bodies;
    n_tiles = e->n_worlds * (int64_t)encounter_tiles((uint32_t)per_world);
    targets = e->n_worlds * per_world;  // (<= 2^26)
  }
  const size_t t = (size_t)targets;
  if (int rc = ens_frame_buffer(e, e->enc_out, e->enc_out_bytes, n * sizeof(nbody_world_encounters))) return rc;
  if (t) {
    if (int rc = ens_frame_buffer(e, e->enc_index, e->enc_index_bytes, t * sizeof(int32_t))) return rc;
    if (int rc = ens_frame_buffer(e, e->enc_d2, e->enc_d2_bytes, t * sizeof(Real))) return rc;
    if (int rc = ens_frame_buffer(e, e->enc_close, e->enc_close_bytes, t * sizeof(uint32_t))) return rc;
    if (int rc = ens_frame_buffer(e, e->enc_live, e->enc_live_bytes, t * sizeof(uint32_t))) return rc;
  }
  if (limit2) {
    if (int rc = ens_frame_buffer(e, e->enc_limit, e->enc_limit_bytes, n * sizeof(float))) return rc;
    ENS_HIPCHK(e, hipMemcpyAsync(e->enc_limit, limit2, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  }
  EncounterArgs a;
  a.pos = e->pos[e->cur];
  a.tpos = rows.tpos;
  a.table = rows.sizes ? e->frame_table : nullptr;
  a.tile_base = rows.sizes ? e->enc_tile_base + (tracers ? n + 1 : 0) : nullptr;
  a.limit2 = limit2 ? e->enc_limit : nullptr;
  a.limit_all = e->params.clamp;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = (uint32_t)rows.n_tracers;
  a.n_worlds = (uint32_t)e->n_worlds;
  a.tracers = tracers ? 1u : 0u;
  a.nn_index = e->enc_index;
  a.nn_d2 = e->enc_d2;
  a.close = e->enc_close;
  a.live = e->enc_live;
  ENS_HIPCHK(e, launch_ensemble_encounters<Real>(e->stream, a, n_tiles, e->enc_out));
  ENS_HIPCHK(e, hipMemcpyAsync(out, e->enc_out, n * sizeof(nbody_world_encounters), hipMemcpyDeviceToHost, e->stream));
  if (t && nn_index) ENS_HIPCHK(e, hipMemcpyAsync(nn_index, e->enc_index, t * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (t && nn_d2) ENS_HIPCHK(e, hipMemcpyAsync(nn_d2, e->enc_d2, t * sizeof(Real), hipMemcpyDeviceToHost, e->stream));
  if (t && close) ENS_HIPCHK(e, hipMemcpyAsync(close, e->enc_close, t * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

#undef ENS_HIPCHK

}  // namespace nbody
