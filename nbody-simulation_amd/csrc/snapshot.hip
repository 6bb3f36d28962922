// libnbody_hip — the current rows handed to the host while steps go on: snapshots (main.rs:136-139), delta snapshots and
// their host decoder (delta_codec.h), and the render entry points.  Kernels: delta_snapshot.hip, render.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "delta_codec.h"
#include "delta_decoder.hpp"
#include "delta_snapshot.h"
#include "driver.h"
#include "render.h"

using namespace nbody;

// A multi-device handle's pending snapshot or stream lives on its first device: taking it does not need the replicas to agree.
#define NB_VIA_FIRST(c, expr)                    \
  do {                                           \
    if ((c)->multi) {                            \
      nbody_ctx* p = nbody::multi_peek(c);       \
      const int rc__ = (expr);                   \
      if (rc__) (c)->err = p->err;               \
      return rc__;                               \
    }                                            \
  } while (0)

// What every call that hands tracers out refuses first: no context, or one that fronts several devices (those hold no tracers).
static int tracers_handoff_check(const nbody_ctx* c, const char* what) {
  if (!c) return fail(nullptr, NBODY_ERR_INVALID, std::string(what) + ": the context is NULL (tracers)");
  if (c->multi)
    return fail(const_cast<nbody_ctx*>(c), NBODY_ERR_INVALID, std::string(what) + ": tracers are not available on a context made by nbody_create_multi");
  return NBODY_OK;
}

// ---- snapshot hand-off (main.rs:136-139) --------------------------------------------------------------------------
void nbody::free_snapshot(nbody_ctx* c) {
  free_dev(c->snap_pos); free_dev(c->snap_vel); free_dev(c->snap_w); free_dev(c->snap_ids);
  free_host(c->snap_hpos); free_host(c->snap_hvel); free_host(c->snap_hw); free_host(c->snap_hids);
  free_dev(c->snap_tpos); free_dev(c->snap_tvel);
  free_host(c->snap_htpos); free_host(c->snap_htvel);
  c->snap_bytes2 = 0;
  c->snap_tcap = 0;
  c->snap_n = 0;
  c->snap_m = 0;
  c->snap_pending = false;
}
template <class T> int snapshot_begin(nbody_ctx* c, State<T>& s) {
  using T2 = typename State<T>::T2;
  const size_t n = (size_t)s.n, b2 = n * sizeof(T2);
  if (c->snap_n != s.n || c->snap_bytes2 != b2) {
    free_snapshot(c);
    if (n) {
      HIPCHK(c, hipMalloc(&c->snap_pos, b2));
      HIPCHK(c, hipMalloc(&c->snap_vel, b2));
      HIPCHK(c, hipMalloc((void**)&c->snap_w, n * 4));
      HIPCHK(c, hipMalloc((void**)&c->snap_ids, n * 4));
      HIPCHK(c, hipHostMalloc(&c->snap_hpos, b2, hipHostMallocDefault));
      HIPCHK(c, hipHostMalloc(&c->snap_hvel, b2, hipHostMallocDefault));
      HIPCHK(c, hipHostMalloc((void**)&c->snap_hw, n * 4, hipHostMallocDefault));
      HIPCHK(c, hipHostMalloc((void**)&c->snap_hids, n * 4, hipHostMallocDefault));
    }
    c->snap_n = s.n;
    c->snap_bytes2 = b2;
  }
  // the tracers the context holds now go with the rows (nbody_snapshot_tracers_*)
  const Tracers& tr = c->tracers;
  const size_t tb = (size_t)tr.m * sizeof(T2);
  if (c->snap_tcap < tb) {
    free_dev(c->snap_tpos); free_dev(c->snap_tvel);
    free_host(c->snap_htpos); free_host(c->snap_htvel);
    c->snap_tcap = 0;
    HIPCHK(c, hipMalloc(&c->snap_tpos, tb));
    HIPCHK(c, hipMalloc(&c->snap_tvel, tb));
    HIPCHK(c, hipHostMalloc(&c->snap_htpos, tb, hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc(&c->snap_htvel, tb, hipHostMallocDefault));
    c->snap_tcap = tb;
  }
  c->snap_f64 = sizeof(T) == 8;
  auto& st = s.set[s.cur];
  // the rows (and the tracers) are copied aside on the stream the steps run on (ordered after the last step, microseconds), so
  // that later steps may overwrite them; the slow leg to the host runs on its own stream, alongside those steps
  if (n) {
    HIPCHK(c, hipMemcpyAsync(c->snap_pos, st.pos, b2, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_vel, st.vel, b2, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_w, st.weight, n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_ids, st.ids, n * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  if (tb) {
    HIPCHK(c, hipMemcpyAsync(c->snap_tpos, tr.pos, tb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_tvel, tr.vel, tb, hipMemcpyDeviceToDevice, c->stream));
  }
  if (n || tb) {
    HIPCHK(c, hipEventRecord(c->snap_event, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->snap_event, 0));
  }
  if (n) {
    HIPCHK(c, hipMemcpyAsync(c->snap_hpos, c->snap_pos, b2, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_hvel, c->snap_vel, b2, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_hw, c->snap_w, n * 4, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_hids, c->snap_ids, n * 4, hipMemcpyDeviceToHost, c->copy_stream));
  }
  if (tb) {
    HIPCHK(c, hipMemcpyAsync(c->snap_htpos, c->snap_tpos, tb, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipMemcpyAsync(c->snap_htvel, c->snap_tvel, tb, hipMemcpyDeviceToHost, c->copy_stream));
  }
  c->snap_m = tr.m;
  c->snap_step = c->steps_done;
  c->snap_pending = true;
  return NBODY_OK;
}
NB_API int nbody_snapshot_begin(nbody_ctx* c) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_PRIMARY(c, false, nbody_snapshot_begin(p));
  if (!c->has_f32 && !c->has_f64) return fail(c, NBODY_ERR_INVALID, "snapshot_begin: no particles uploaded");
  if (c->snap_pending) return fail(c, NBODY_ERR_INVALID, "snapshot_begin: a snapshot is still pending (take it with nbody_snapshot_end)");
  HIPCHK(c, hipSetDevice(c->device));
  return c->has_f32 ? snapshot_begin<float>(c, c->sf) : snapshot_begin<double>(c, c->sd);
}
NB_API int nbody_snapshot_pending(const nbody_ctx* c) {
  if (c && c->multi) return nbody_snapshot_pending(nbody::multi_peek(c));
  return c && c->snap_pending ? 1 : 0;
}
static int snapshot_end(nbody_ctx* c, bool f64, void* pos, void* vel, uint32_t* w, uint32_t* ids, uint64_t* step) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_FIRST(c, snapshot_end(p, f64, pos, vel, w, ids, step));
  if (!c->snap_pending) return fail(c, NBODY_ERR_INVALID, "snapshot_end: no snapshot pending");
  if (c->snap_f64 != f64) return fail(c, NBODY_ERR_INVALID, "snapshot_end: the pending snapshot has the other precision");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  const size_t n = (size_t)c->snap_n;
  if (n) {
    if (pos) std::memcpy(pos, c->snap_hpos, c->snap_bytes2);
    if (vel) std::memcpy(vel, c->snap_hvel, c->snap_bytes2);
    if (w) std::memcpy(w, c->snap_hw, n * 4);
    if (ids) std::memcpy(ids, c->snap_hids, n * 4);
  }
  if (step) *step = c->snap_step;
  c->snap_pending = false;
  return NBODY_OK;
}
NB_API int nbody_snapshot_end_f32(nbody_ctx* c, float* pos, float* vel, uint32_t* w, uint32_t* ids, uint64_t* step) {
  return snapshot_end(c, false, pos, vel, w, ids, step);
}
NB_API int nbody_snapshot_end_f64(nbody_ctx* c, double* pos, double* vel, uint32_t* w, uint32_t* ids, uint64_t* step) {
  return snapshot_end(c, true, pos, vel, w, ids, step);
}

NB_API int64_t nbody_snapshot_num_tracers(const nbody_ctx* c) {
  const int rc = tracers_handoff_check(c, "snapshot_num_tracers");
  if (rc) return rc;
  return c->snap_pending ? c->snap_m : 0;
}
// The pending snapshot's tracers: as they were at begin, whatever happened to the context's tracers since.  Does not end the snapshot.
static int snapshot_tracers(nbody_ctx* c, bool f64, void* pos, void* vel) {
  const int rc = tracers_handoff_check(c, "snapshot_tracers");
  if (rc) return rc;
  if (!c->snap_pending) return fail(c, NBODY_ERR_INVALID, "snapshot_tracers: no snapshot pending");
  if (c->snap_f64 != f64) return fail(c, NBODY_ERR_INVALID, "snapshot_tracers: the pending snapshot has the other precision");
  if (c->snap_m == 0) return NBODY_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  const size_t tb = (size_t)c->snap_m * 2 * (f64 ? sizeof(double) : sizeof(float));
  if (pos) std::memcpy(pos, c->snap_htpos, tb);
  if (vel) std::memcpy(vel, c->snap_htvel, tb);
  return NBODY_OK;
}
NB_API int nbody_snapshot_tracers_f32(nbody_ctx* c, float* pos, float* vel) { return snapshot_tracers(c, false, pos, vel); }
NB_API int nbody_snapshot_tracers_f64(nbody_ctx* c, double* pos, double* vel) { return snapshot_tracers(c, true, pos, vel); }

// ---- delta snapshots (the commented experiment of main.rs:107-134; format: delta_codec.h) -------------------------
static void free_delta_stream(DeltaStream& d) {
  for (auto& k : d.keys) free_dev(k);
  free_dev(d.widths); free_dev(d.words); free_dev(d.offsets); free_dev(d.scan); free_dev(d.payload);
  free_dev(d.total);
  free_host(d.host); free_host(d.htotal);
  d.n = -1;
  d.bits = 0;
  d.key_next = true;
  d.pending = false;
}
void nbody::free_delta(nbody_ctx* c) {
  free_delta_stream(c->dl);
  free_delta_stream(c->tdl);
}
// One stream of the sequence `d`: n positions of precision T, put in id order by `ids` (nullptr: they are in id order).
template <class T> int delta_begin(nbody_ctx* c, DeltaStream& d, int64_t n, const void* pos, const uint32_t* ids) {
  const int bits = (int)sizeof(T) * 8;
  const size_t nblk = delta_blocks(n), npad = nblk * 64, kb = 2 * npad * sizeof(T), wb = delta_width_bytes(n);
  if (d.n != n || d.bits != bits) {
    free_delta_stream(d);
    for (auto& k : d.keys) HIPCHK(c, hipMalloc(&k, kb ? kb : 8));
    HIPCHK(c, hipMalloc((void**)&d.widths, wb ? wb : 8));
    HIPCHK(c, hipMalloc((void**)&d.words, 2 * nblk * 4 + 8));
    HIPCHK(c, hipMalloc((void**)&d.offsets, 2 * nblk * 4 + 8));
    d.scan_bytes = delta_scan_temp_bytes(n);
    HIPCHK(c, hipMalloc(&d.scan, d.scan_bytes ? d.scan_bytes : 8));
    HIPCHK(c, hipMalloc((void**)&d.payload, 2 * nblk * (size_t)bits * 8 + 8));
    HIPCHK(c, hipMalloc((void**)&d.total, 8));
    HIPCHK(c, hipHostMalloc((void**)&d.host, delta_bound(n, bits), hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void**)&d.htotal, 8, hipHostMallocDefault));
    if (wb) HIPCHK(c, hipMemsetAsync(d.widths, 0, wb, c->stream));  // the padding bytes stay zero
    d.n = n;
    d.bits = bits;
    d.key_next = true;
  }
  const bool key = d.key_next;
  if (key && kb)
    for (auto& k : d.keys) HIPCHK(c, hipMemsetAsync(k, 0, kb, c->stream));
  void* cur = d.keys[d.cur];
  const void* prev = d.keys[(d.cur + 2) % 3];
  const void* prev2 = d.keys[(d.cur + 1) % 3];
  HIPCHK(c, launch_delta_encode<T>(c->stream, n, pos, ids, cur, prev, prev2, d.widths, d.words, d.offsets, d.scan, d.scan_bytes,
                                   d.payload, d.total));
  HIPCHK(c, hipEventRecord(c->snap_event, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->snap_event, 0));
  // the size of the stream is known on the device only: fetch it, then start the transfer proper (which later steps overlap)
  HIPCHK(c, hipMemcpyAsync(d.htotal, d.total, 8, hipMemcpyDeviceToHost, c->copy_stream));
  HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  const uint64_t total = *d.htotal;
  if (total > 2 * nblk * (uint64_t)bits) return fail(c, NBODY_ERR_HIP, "delta_begin: the encoder reported an impossible size");
  uint8_t* h = d.host;
  std::memset(h, 0, kDeltaHeader);
  h[0] = 'N'; h[1] = 'B'; h[2] = 'D'; h[3] = '1';
  h[4] = (uint8_t)bits;
  h[5] = key ? 1 : 0;
  const uint64_t n64 = (uint64_t)n, step = c->steps_done;
  std::memcpy(h + 8, &n64, 8);
  std::memcpy(h + 16, &step, 8);
  std::memcpy(h + 24, &total, 8);
  if (wb) HIPCHK(c, hipMemcpyAsync(h + kDeltaHeader, d.widths, wb, hipMemcpyDeviceToHost, c->copy_stream));
  if (total) HIPCHK(c, hipMemcpyAsync(h + kDeltaHeader + wb, d.payload, total * 8, hipMemcpyDeviceToHost, c->copy_stream));
  d.stream_bytes = kDeltaHeader + wb + (size_t)total * 8;
  d.cur = (d.cur + 1) % 3;  // the oldest keys are overwritten next time
  d.key_next = false;
  d.step = step;
  d.pending = true;
  return NBODY_OK;
}
static int delta_end(nbody_ctx* c, DeltaStream& d, const char* what, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* step_out) {
  if (!d.pending) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": no stream pending");
  if (bytes_out) *bytes_out = d.stream_bytes;
  if (step_out) *step_out = d.step;
  if (!out || cap < d.stream_bytes) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": the output buffer is smaller than the stream");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  std::memcpy(out, d.host, d.stream_bytes);
  d.pending = false;
  return NBODY_OK;
}
NB_API int nbody_delta_begin(nbody_ctx* c) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_PRIMARY(c, false, nbody_delta_begin(p));
  if (!c->has_f32 && !c->has_f64) return fail(c, NBODY_ERR_INVALID, "delta_begin: no particles uploaded");
  if (c->dl.pending) return fail(c, NBODY_ERR_INVALID, "delta_begin: a stream is still pending (take it with nbody_delta_end)");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->has_f32) {
    auto& st = c->sf.set[c->sf.cur];
    return delta_begin<float>(c, c->dl, c->sf.n, st.pos, st.ids);
  }
  auto& st = c->sd.set[c->sd.cur];
  return delta_begin<double>(c, c->dl, c->sd.n, st.pos, st.ids);
}
NB_API int nbody_delta_pending(const nbody_ctx* c) {
  if (c && c->multi) return nbody_delta_pending(nbody::multi_peek(c));
  return c && c->dl.pending ? 1 : 0;
}
NB_API int nbody_delta_end(nbody_ctx* c, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* step_out) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_FIRST(c, nbody_delta_end(p, out, cap, bytes_out, step_out));
  return delta_end(c, c->dl, "delta_end", out, cap, bytes_out, step_out);
}
NB_API int nbody_delta_reset(nbody_ctx* c) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_FIRST(c, nbody_delta_reset(p));
  if (c->dl.pending) return fail(c, NBODY_ERR_INVALID, "delta_reset: a stream is still pending");
  c->dl.key_next = true;
  return NBODY_OK;
}

// The tracers' positions as a second sequence of the same format: the header's count is m, the order the upload's.
NB_API int nbody_tracers_delta_begin(nbody_ctx* c) {
  const int rc = tracers_handoff_check(c, "tracers_delta_begin");
  if (rc) return rc;
  if (c->tracers.m == 0) return fail(c, NBODY_ERR_INVALID, "tracers_delta_begin: the context holds no tracers");
  if (c->tdl.pending)
    return fail(c, NBODY_ERR_INVALID, "tracers_delta_begin: a tracers stream is still pending (take it with nbody_tracers_delta_end)");
  HIPCHK(c, hipSetDevice(c->device));
  return c->has_f32 ? delta_begin<float>(c, c->tdl, c->tracers.m, c->tracers.pos, nullptr)
                    : delta_begin<double>(c, c->tdl, c->tracers.m, c->tracers.pos, nullptr);
}
NB_API int nbody_tracers_delta_pending(const nbody_ctx* c) {
  const int rc = tracers_handoff_check(c, "tracers_delta_pending");
  if (rc) return rc;
  return c->tdl.pending ? 1 : 0;
}
NB_API int nbody_tracers_delta_end(nbody_ctx* c, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* step_out) {
  const int rc = tracers_handoff_check(c, "tracers_delta_end");
  if (rc) return rc;
  return delta_end(c, c->tdl, "tracers_delta_end", out, cap, bytes_out, step_out);
}
NB_API int nbody_tracers_delta_reset(nbody_ctx* c) {
  const int rc = tracers_handoff_check(c, "tracers_delta_reset");
  if (rc) return rc;
  if (c->tdl.pending) return fail(c, NBODY_ERR_INVALID, "tracers_delta_reset: a tracers stream is still pending");
  c->tdl.key_next = true;
  return NBODY_OK;
}
NB_API size_t nbody_delta_bound(int64_t n, int is_f64) { return n < 0 ? 0 : delta_bound(n, is_f64 ? 64 : 32); }

// The receiving side: plain host code (delta_decoder.hpp; the consumer of a snapshot is a host thread, main.rs:147-150).
struct nbody_delta_decoder {
  DeltaDecoder d;
};
NB_API nbody_delta_decoder* nbody_delta_decoder_create(void) { return new (std::nothrow) nbody_delta_decoder(); }
NB_API void nbody_delta_decoder_destroy(nbody_delta_decoder* d) { delete d; }
NB_API const char* nbody_delta_decoder_error(const nbody_delta_decoder* d) { return d ? d->d.err.c_str() : "null decoder"; }
NB_API int64_t nbody_delta_decoder_count(const nbody_delta_decoder* d) { return d ? d->d.n : -1; }
NB_API int nbody_delta_decoder_is_f64(const nbody_delta_decoder* d) { return d && d->d.bits == 64 ? 1 : 0; }
NB_API uint64_t nbody_delta_decoder_step(const nbody_delta_decoder* d) { return d ? d->d.step : 0; }
NB_API int nbody_delta_decoder_apply(nbody_delta_decoder* d, const uint8_t* stream, size_t bytes) {
  if (!d) return NBODY_ERR_INVALID;
  try {  // nothing may unwind through the C ABI (the decoder itself already turns a failed allocation into a refusal)
    return d->d.apply(stream, bytes) ? NBODY_OK : NBODY_ERR_INVALID;
  } catch (...) {
    return NBODY_ERR_NOMEM;
  }
}
NB_API int nbody_delta_decoder_set_max_bodies(nbody_delta_decoder* d, int64_t max_bodies) {
  if (!d || max_bodies < 0) return NBODY_ERR_INVALID;
  d->d.max_bodies = (uint64_t)max_bodies;
  return NBODY_OK;
}
NB_API int nbody_delta_decoder_positions_f32(const nbody_delta_decoder* d, float* pos) {
  return d && d->d.positions<float, uint32_t>(pos) ? NBODY_OK : NBODY_ERR_INVALID;
}
NB_API int nbody_delta_decoder_positions_f64(const nbody_delta_decoder* d, double* pos) {
  return d && d->d.positions<double, uint64_t>(pos) ? NBODY_OK : NBODY_ERR_INVALID;
}

template <class T> int render_rows(nbody_ctx* c, State<T>& s, bool tracers, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  auto& st = s.set[s.cur];
  const Tracers& tr = c->tracers;
  HIPCHK(c, launch_render_tracers<T>(c->stream, s.n, st.pos, st.vel, st.weight, tracers ? tr.m : 0, tr.pos, tr.vel, height, render_px,
                                     c->frame_work, c->frame_rgba));
  HIPCHK(c, hipMemcpyAsync(rgba_out, c->frame_rgba, (size_t)render_px * render_px * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}
// What nbody_render_rgba and nbody_render_rgba_tracers share, past the handle: the arguments, the frame's buffers, the frame.
static int render_frame(nbody_ctx* c, bool tracers, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  if (!rgba_out) return fail(c, NBODY_ERR_INVALID, "render: null output");
  if (!c->has_f32 && !c->has_f64) return fail(c, NBODY_ERR_INVALID, "render: no particles uploaded");
  // main.rs:51-52 divide by HEIGHT / RENDER_HEIGHT: a cell of 0 world units or a last cell past the frame is an
  // out-of-range index upstream (a panic): refuse instead
  if (render_px == 0 || render_px > 16384 || height == 0 || height % render_px != 0 || height > (1u << 24))
    return fail(c, NBODY_ERR_INVALID, "render: render_px must divide height (both > 0, height <= 2^24, render_px <= 16384)");
  const int64_t n = c->has_f32 ? c->sf.n : c->sd.n;
  if (n > (1 << 24)) return fail(c, NBODY_ERR_INVALID, "render: more than 2^24 rows");
  if (tracers && n + c->tracers.m > (1 << 24)) return fail(c, NBODY_ERR_INVALID, "render: more than 2^24 rows, bodies and tracers together");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->frame_px != render_px) {
    free_dev(c->frame_work); free_dev(c->frame_rgba);
    c->frame_px = 0;
    HIPCHK(c, hipMalloc((void**)&c->frame_work, sizeof(uint32_t) * 2 * (size_t)render_px * render_px));
    HIPCHK(c, hipMalloc((void**)&c->frame_rgba, (size_t)render_px * render_px * 4));
    c->frame_px = render_px;
  }
  return c->has_f32 ? render_rows<float>(c, c->sf, tracers, height, render_px, rgba_out)
                    : render_rows<double>(c, c->sd, tracers, height, render_px, rgba_out);
}
NB_API int nbody_render_rgba(nbody_ctx* c, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_PRIMARY(c, false, nbody_render_rgba(p, height, render_px, rgba_out));
  return render_frame(c, false, height, render_px, rgba_out);
}
NB_API int nbody_render_rgba_tracers(nbody_ctx* c, uint32_t height, uint32_t render_px, uint8_t* rgba_out) {
  const int rc = tracers_handoff_check(c, "render");
  if (rc) return rc;
  return render_frame(c, true, height, render_px, rgba_out);
}
NB_API int nbody_render_rgba_dev(void* stream, int64_t n, int is_f64, const void* pos_xy, const void* vel_xy, const void* weight_u32,
                                 uint32_t height, uint32_t render_px, void* work_u32, void* rgba_dev) {
  if (n < 0 || n > (1 << 24) || render_px == 0 || height == 0 || height % render_px != 0 || height > (1u << 24) || !work_u32 || !rgba_dev ||
      (n > 0 && (!pos_xy || !vel_xy || !weight_u32)))
    return NBODY_ERR_INVALID;
  hipError_t e = is_f64 ? launch_render<double>((hipStream_t)stream, n, pos_xy, vel_xy, (const uint32_t*)weight_u32, height, render_px,
                                                (uint32_t*)work_u32, (uint8_t*)rgba_dev)
                        : launch_render<float>((hipStream_t)stream, n, pos_xy, vel_xy, (const uint32_t*)weight_u32, height, render_px,
                                               (uint32_t*)work_u32, (uint8_t*)rgba_dev);
  return e == hipSuccess ? NBODY_OK : NBODY_ERR_HIP;
}
