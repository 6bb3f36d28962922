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
//   launch(stream, n_worlds, args) one step, or one force evaluation, of all worlds;
//   launch_resident(stream, n_worlds, worlds, lds_bytes, args), resident_lds_bytes(n_bodies)
//                                  resident runs (ens_resident_with): one launch of ensemble_resident.h and a world's dynamic LDS in it.
// A handle is a struct of its own derived from EnsembleState<P>: the C header declares distinct opaque types.
// The ragged handle (ragged_driver.h: worlds of different sizes, several launches per step) is built from the same parts: the
// state, create / destroy, params and errors as they are, and upload, download, update and accel through the *_rows / *_with
// functions below, which take the number of rows and the step's launches from their caller.
// The restricted handle (restricted_driver.h: tracers beside the bodies, a second launch per step) is the whole of this driver
// under its own kWho, with the tracers' launch added to a step through ens_update_with.
// This file: the state (with the scratch of every call, each a DevBuf grown on demand and freed with the rows), create /
// destroy, params, upload / download, and the stepping calls: update, sweep (nbody_sweep_*: a time step, a clamp and a number of
// steps per world), resident (nbody_resident_*: that sweep with every world kept in LDS for up to 1024 steps of a launch) and
// accel; ens_enqueue_step and ens_enqueue_sweep_step are one step of either kind, for the watched runs too.
// The calls that read every world's current rows and return something per world — frames, delta streams, summaries, encounters
// — and the watched runs are ensemble_observers.h, included at the end: one function each for every handle, told where the
// handle's rows are by one WorldRows.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "driver.h"
#include "ensemble_deltas.h"
#include "ensemble_kernels.h"
#include "ensemble_resident.h"
#include "ensemble_rows.h"
#include "ensemble_watch.h"

namespace nbody {

template <class P> struct EnsembleState;

// A device scratch buffer of a handle: grown to what a call needs, never shrunk, freed with the handle's rows.
template <class T> struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  template <class P> int grow(EnsembleState<P>* e, size_t need);  // (below) at least `need` bytes; a smaller buffer is freed and replaced
  void release() {
    free_dev(p);
    bytes = 0;
  }
};

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
  DevBuf<uint8_t> out;         // grown to the streams of a call
  void release() {
    for (auto& k : keys) free_dev(k);
    free_dev(widths); free_dev(words); free_dev(offsets); free_dev(scan); free_dev(table); free_dev(seg_of_block);
    free_dev(stream_off);
    out.release();
    *this = DeltaSeq();
  }
};

// A ragged handle's table of row ranges on the device and what hangs off it: for the summaries the first chunk of every world's
// tracers among the chunks of all worlds' tracers, and their total; for the encounters the first tile of every world's bodies
// among the tiles of all worlds' bodies, the same for the tracers, and the two totals.  Built (ens_world_table,
// ensemble_observers.h) by the first frames, summary or encounters call after an upload of bodies or tracers; the arrays are
// allocated once per upload of the bodies and freed with them.
struct WorldTable {
  WorldRanges* worlds = nullptr;           // [n_worlds]
  uint32_t* summary_chunk_base = nullptr;  // [n_worlds + 1]
  uint32_t* enc_tile_base = nullptr;       // [2][n_worlds + 1]: the bodies', then the tracers'
  int64_t summary_tracer_chunks = 0, enc_body_tiles = 0, enc_tracer_tiles = 0;
  bool valid = false;
  void invalidate() { valid = false; }     // (the arrays stay: the next build overwrites them)
  void release() {
    free_dev(worlds); free_dev(summary_chunk_base); free_dev(enc_tile_base);
    *this = WorldTable();
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
  // Everything below is scratch of the calls named, freed with the arrays above (ens_free).
  WorldTable table;  // a ragged handle's row ranges, for frames, summaries and encounters
  // frames (ens_frames)
  DevBuf<uint8_t> frame_rgba;
  DevBuf<uint32_t> frame_work;
  // delta streams (ens_deltas): the steps taken since the handle was created (it runs on across uploads, as a context's count
  // does), and the two sequences.  The bodies' goes with the arrays above; the tracers' with the tracers of the handles that
  // have them (and so with the bodies too: an upload of bodies removes the tracers).
  uint64_t updates = 0;
  DeltaSeq dbodies, dtracers;
  // sweeps (ens_sweep_with): the table of the worlds' entries of the call in flight, on the host and on the device; rewritten by
  // every call, nothing of a sweep outlives it
  std::vector<typename P::SweepWorld> sweep_host;
  DevBuf<typename P::SweepWorld> sweep_dev;
  // resident runs (ens_resident_with) of a ragged handle: every world's {row0, n}, made by the first such call after an upload
  std::vector<uint2> resident_host;
  DevBuf<uint2> resident_worlds;
  // summaries (ens_summary): the records, the chunk records of segments of several chunks and the call's ref[]
  DevBuf<nbody_world_summary> summary_out, summary_chunks;
  DevBuf<int32_t> summary_ref;
  // encounters (ens_encounters): the records, the four per-target arrays and the call's limit2[]
  DevBuf<nbody_world_encounters> enc_out;
  DevBuf<int32_t> enc_index;
  DevBuf<typename P::Real> enc_d2;
  DevBuf<uint32_t> enc_close, enc_live;
  DevBuf<float> enc_limit;
  // a watched run (ens_watch_with): the records, the six running rows per target and the call's limit2[]
  DevBuf<nbody_world_watch> watch_out;
  DevBuf<typename P::Real> watch_d2;
  DevBuf<int32_t> watch_index;
  DevBuf<uint32_t> watch_sample, watch_first_close, watch_close_samples, watch_first_out;
  DevBuf<float> watch_limit;
  // a watched sweep (ens_wsweep_with): the watch's scratch above, the sweep's table, and every world's sampling schedule
  std::vector<WatchWorld> watch_sched_host;
  DevBuf<WatchWorld> watch_sched;
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

template <class T> template <class P> int DevBuf<T>::grow(EnsembleState<P>* e, size_t need) {
  if (bytes >= need) return NBODY_OK;
  free_dev(p);
  bytes = 0;
  ENS_HIPCHK(e, hipMalloc((void**)&p, need));
  bytes = need;
  return NBODY_OK;
}

template <class P> void ens_free(EnsembleState<P>* e) {
  free_dev(e->pos[0]); free_dev(e->pos[1]); free_dev(e->vel); free_dev(e->mass); free_dev(e->acc);
  e->table.release();
  e->frame_rgba.release(); e->frame_work.release();
  e->sweep_dev.release();
  e->resident_worlds.release();
  e->summary_out.release(); e->summary_chunks.release(); e->summary_ref.release();
  e->enc_out.release(); e->enc_index.release(); e->enc_d2.release(); e->enc_close.release(); e->enc_live.release(); e->enc_limit.release();
  e->watch_out.release(); e->watch_d2.release(); e->watch_index.release(); e->watch_sample.release(); e->watch_first_close.release();
  e->watch_close_samples.release(); e->watch_first_out.release(); e->watch_limit.release(); e->watch_sched.release();
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

// One step by `delta` enqueued through `launch(args)`: what an update and a watched run (ens_watch_with, ensemble_observers.h)
// do per step.
template <class P, class Launch> hipError_t ens_enqueue_step(EnsembleState<P>* e, typename P::Real delta, Launch& launch) {
  typename P::Args a = ens_args(e);
  a.pos_out = e->pos[1 - e->cur];
  a.vel = e->vel;
  a.delta = delta;
  const hipError_t h = launch(a);
  if (h != hipSuccess) return h;
  e->cur = 1 - e->cur;  // (the launches are in stream order: the next one reads what this one writes)
  ++e->updates;
  return hipSuccess;
}

// Step `step` of a sweep whose table is in e->sweep_dev, enqueued through `launch(args)`: what a sweep and a watched sweep
// (ens_wsweep_with, ensemble_observers.h) do per step.  own_clamp: the call brought a clamp per world.
template <class P, class Launch> hipError_t ens_enqueue_sweep_step(EnsembleState<P>* e, bool own_clamp, int step, Launch& launch) {
  typename P::Args a = ens_args(e);
  if (own_clamp) P::sweep_route(a, e->params);
  a.pos_out = e->pos[1 - e->cur];
  a.vel = e->vel;
  a.sweep = e->sweep_dev.p;
  a.step = step;
  const hipError_t h = launch(a);
  if (h != hipSuccess) return h;
  e->cur = 1 - e->cur;
  ++e->updates;
  return hipSuccess;
}

// The worlds' entries of a sweep's table from the call's arrays, on their way to the device (the copy is enqueued, not waited for).
template <class P> int ens_sweep_table(EnsembleState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps) {
  const size_t n = (size_t)e->n_worlds, bytes = n * sizeof(typename P::SweepWorld);
  e->sweep_host.resize(n);  // (the handle's: the copy below may still read it when an error returns early)
  for (size_t k = 0; k < n; ++k) e->sweep_host[k] = P::sweep_world(delta[k], clamp ? clamp[k] : e->params.clamp, steps ? steps[k] : n_steps);
  if (int rc = e->sweep_dev.grow(e, bytes)) return rc;
  const hipError_t h = hipMemcpyAsync(e->sweep_dev.p, e->sweep_host.data(), bytes, hipMemcpyHostToDevice, e->stream);
  return h == hipSuccess ? NBODY_OK : ens_fail_hip<P>(e, h, "upload of the sweep's table");
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
  for (int step = 0; step < n_steps; ++step) ENS_HIPCHK(e, ens_enqueue_step(e, delta, launch));
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

// What a sweep refuses of its arguments, for `who` ("<handle's word> sweep: ", or the resident run's): nothing uploaded, no
// delta, n_steps < 0, a steps[k] outside 0 .. n_steps.
template <class P>
int ens_sweep_check(EnsembleState<P>* e, const std::string& who, const typename P::Real* delta, const int32_t* steps, int n_steps) {
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!delta) return ens_fail(e, NBODY_ERR_INVALID, who + "delta is NULL");
  if (n_steps < 0) return ens_fail(e, NBODY_ERR_INVALID, who + "n_steps < 0");
  if (steps)
    for (int64_t k = 0; k < e->n_worlds; ++k)
      if (steps[k] < 0 || steps[k] > n_steps)
        return ens_fail(e, NBODY_ERR_INVALID, who + "steps[" + std::to_string(k) + "] = " + std::to_string(steps[k]) + " of world " +
                                                  std::to_string(k) + " is outside 0 .. n_steps = " + std::to_string(n_steps));
  return NBODY_OK;
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
  if (int rc = ens_sweep_check(e, std::string(P::kWho) + " sweep: ", delta, steps, n_steps)) return rc;
  if (n_steps == 0) return NBODY_OK;
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  if (int rc = ens_sweep_table(e, delta, clamp, steps, n_steps)) return rc;
  for (int step = 0; step < n_steps; ++step) ENS_HIPCHK(e, ens_enqueue_sweep_step(e, clamp != nullptr, step, launch));
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

// A resident run (nbody_resident_*): the sweep above through another route — one block per world keeps its world in LDS and
// takes up to kResidentStepsPerLaunch of its steps per launch (ensemble_resident.h), so a call whose largest steps[k] is S
// enqueues ceil(S / kResidentStepsPerLaunch) launches instead of n_steps.  The arguments and their checks are the sweep's, the
// table is the sweep's (ens_sweep_table), and so are the arithmetic of a launch and the bookkeeping: the handle's step count
// advances by n_steps, the seconds go to sum_gravity.  The kernels write the rows in place, so the position buffers do not flip.
// sizes: the bodies per world of a ragged handle, or NULL (e->n_bodies in every world).  Every refusal comes before anything is
// allocated or enqueued.
template <class P>
int ens_resident_with(EnsembleState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps,
                      nbody_counting* counter, const int64_t* sizes = nullptr) {
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " resident: ";
  if (int rc = ens_sweep_check(e, who, delta, steps, n_steps)) return rc;
  int32_t most = steps ? 0 : n_steps;
  if (steps)
    for (int64_t k = 0; k < e->n_worlds; ++k) most = std::max(most, steps[k]);
  int64_t largest = e->n_bodies;
  for (int64_t k = 0; k < e->n_worlds; ++k) {
    const int64_t n = sizes ? sizes[k] : e->n_bodies;
    if (n > kResidentMaxBodies)
      return ens_fail(e, NBODY_ERR_INVALID, who + "world " + std::to_string(k) + " has " + std::to_string(n) + " bodies; a resident run takes worlds of at most " +
                                                std::to_string(kResidentMaxBodies) + " (one block per world): sweep is the call for this handle");
    if (n > largest) largest = n;
    if (!sizes) break;  // (worlds of one size)
  }
  if (n_steps == 0) return NBODY_OK;
  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  if (most > 0) {
    if (int rc = ens_sweep_table(e, delta, clamp, steps, n_steps)) return rc;
    if (sizes && !e->resident_worlds.p) {
      const size_t n = (size_t)e->n_worlds;
      e->resident_host.resize(n);  // (the handle's: the copy below may still read it when an error returns early)
      uint32_t row0 = 0;
      for (size_t k = 0; k < n; ++k) {
        e->resident_host[k] = uint2{row0, (uint32_t)sizes[k]};
        row0 += (uint32_t)sizes[k];  // (rows of all worlds <= 2^26)
      }
      if (int rc = e->resident_worlds.grow(e, n * sizeof(uint2))) return rc;
      const hipError_t h = hipMemcpyAsync(e->resident_worlds.p, e->resident_host.data(), n * sizeof(uint2), hipMemcpyHostToDevice, e->stream);
      if (h != hipSuccess) {
        e->resident_worlds.release();  // (not filled: the next call makes it again)
        return ens_fail_hip<P>(e, h, "upload of the resident run's table");
      }
    }
    typename P::Args a = ens_args(e);
    if (clamp) P::sweep_route(a, e->params);
    a.vel = e->vel;
    a.sweep = e->sweep_dev.p;
    const size_t lds = P::resident_lds_bytes((int)largest);
    for (int64_t base = 0; base < most; base += kResidentStepsPerLaunch) {
      a.step = (int)base;
      ENS_HIPCHK(e, P::launch_resident(e->stream, e->n_worlds, sizes ? e->resident_worlds.p : nullptr, lds, a));
    }
  }
  e->updates += (uint64_t)n_steps;  // the handle's steps, as after the sweep: not any world's own
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  const double dt = now_s() - t_begin;  // booked as an update's seconds are
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
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

}  // namespace nbody

#include "ensemble_observers.h"  // (frames, delta streams, summaries, encounters and the watched run of the state above)
