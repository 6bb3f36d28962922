// libnbody_hip — ensembles: the observers, the calls that read every world's current rows and return something per world, written
// once over a precision P for every handle of ensemble_driver.h (which includes this file at its end).  Internal.
//   ens_frames      nbody_frames_*      every world's draw() raster                        (ensemble_frames.h)
//   ens_deltas      nbody_deltas_*      every world's NBD1 delta stream                    (ensemble_deltas.h)
//   ens_summary     nbody_summary_*     one nbody_world_summary per world                  (ensemble_summary.h)
//   ens_encounters  nbody_encounters_*  nearest neighbours and clamped pairs per world     (ensemble_encounters.h)
// Each is synchronous on the handle's stream, writes no simulation state, refuses before it allocates or launches anything, and
// keeps its device scratch in the state.  And the one call that observes while it steps:
//   ens_watch_with  nbody_watch_*       an update sampled before, between and after its steps    (ensemble_watch.h)
//   ens_wsweep_with nbody_wsweep_*      a sweep sampled so, on every world's own schedule        (ensemble_watch.h)
// What differs between the handles is where their rows are: one WorldRows, which the
// ragged, restricted and ragged restricted drivers each make in one function (ragged_rows, rst_rows, rr_rows).  What a call
// wants of those rows — the bodies or the tracers, the tracers painted or not — is the call's own argument.
#pragma once
#include <algorithm>
#include <limits>
#include <type_traits>

#include "ensemble_driver.h"
#include "ensemble_encounters.h"
#include "ensemble_frames.h"
#include "ensemble_summary.h"
#include "ensemble_watch.h"
#include "env.h"

namespace nbody {

// Where a handle's bodies and tracers are, beyond the bodies of worlds of one size (the default: the plain ensemble's).
template <class P> struct WorldRows {
  const int64_t* sizes = nullptr;         // worlds of different sizes: the bodies per world; NULL: e->n_bodies in every world
  const int64_t* counts = nullptr;        // with sizes: the tracers per world, or NULL: none
  int64_t n_tracers = 0;                  // without sizes: the tracers per world
  int64_t tracer_rows = 0;                // the tracers of all worlds together
  const typename P::Vec2* tpos = nullptr; // the tracers (NULL where the handle holds none)
  const typename P::Vec2* tvel = nullptr;
  bool has_tracer_calls = false;          // the handle's kind has tracer calls at all: the *_TRACERS flags are its to ask
};

// A ragged handle's table (WorldTable, ensemble_driver.h) brought up to its sizes and counts: a no-op while it is valid.
template <class P> int ens_world_table(EnsembleState<P>* e, const WorldRows<P>& rows) {
  WorldTable& t = e->table;
  if (t.valid) return NBODY_OK;
  const size_t n = (size_t)e->n_worlds;
  std::vector<WorldRanges> worlds(n);
  std::vector<uint32_t> chunk_base(n + 1), tile_base(2 * (n + 1));
  int64_t row0 = 0, trow0 = 0, chunk0 = 0, tile0 = 0, ttile0 = 0;
  for (size_t k = 0; k < n; ++k) {
    const int64_t m = rows.counts ? rows.counts[k] : 0;
    worlds[k] = WorldRanges{(uint32_t)row0, (uint32_t)rows.sizes[k], (uint32_t)trow0, (uint32_t)m};  // (each sum <= 2^26)
    chunk_base[k] = (uint32_t)chunk0;                                                                 // (<= 2^26 worlds + 2^14 full chunks)
    row0 += rows.sizes[k];
    trow0 += m;
    chunk0 += summary_chunks((uint32_t)m);
    tile_base[k] = (uint32_t)tile0;                                                                   // (<= 2^26 worlds + 2^18 full tiles)
    tile_base[n + 1 + k] = (uint32_t)ttile0;
    tile0 += encounter_tiles((uint32_t)rows.sizes[k]);
    ttile0 += encounter_tiles((uint32_t)m);
  }
  chunk_base[n] = (uint32_t)chunk0;
  tile_base[n] = (uint32_t)tile0;
  tile_base[2 * n + 1] = (uint32_t)ttile0;
  if (!t.worlds) ENS_HIPCHK(e, hipMalloc((void**)&t.worlds, n * sizeof(WorldRanges)));
  if (!t.summary_chunk_base) ENS_HIPCHK(e, hipMalloc((void**)&t.summary_chunk_base, (n + 1) * sizeof(uint32_t)));
  ENS_HIPCHK(e, hipMemcpyAsync(t.worlds, worlds.data(), n * sizeof(WorldRanges), hipMemcpyHostToDevice, e->stream));
  if (!t.enc_tile_base) ENS_HIPCHK(e, hipMalloc((void**)&t.enc_tile_base, 2 * (n + 1) * sizeof(uint32_t)));
  ENS_HIPCHK(e, hipMemcpyAsync(t.summary_chunk_base, chunk_base.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  ENS_HIPCHK(e, hipMemcpyAsync(t.enc_tile_base, tile_base.data(), 2 * (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));  // (the vectors go out of scope)
  t.summary_tracer_chunks = chunk0;
  t.enc_body_tiles = tile0;
  t.enc_tracer_tiles = ttile0;
  t.valid = true;
  return NBODY_OK;
}

// ---- frames: every world's draw() raster (ensemble_frames.h) of the current positions, into host memory
// rgba_out: [n_worlds][render_px][render_px][4] bytes.  with_tracers: every world's tracers are painted after its bodies, where
// the handle holds any (the table of a ragged handle keeps the counts either way).  Reads pos[cur] and the tracers.
template <class P>
int ens_frames(EnsembleState<P>* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out, const WorldRows<P>& rows = WorldRows<P>(),
               bool with_tracers = false) {
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
  const bool tracers = with_tracers && rows.tracer_rows > 0;
  int64_t max_rows = e->n_bodies + (tracers ? rows.n_tracers : 0);
  if (rows.sizes)
    for (int64_t k = 0; k < e->n_worlds; ++k) max_rows = std::max(max_rows, rows.sizes[k] + (tracers && rows.counts ? rows.counts[k] : 0));
  // (a world has at most 4096 bodies: only the sum with its tracers can pass 2^24)
  if (max_rows > kFrameMaxRows)
    return ens_fail(e, NBODY_ERR_INVALID, who + "a world's bodies and tracers together must be <= 2^24 rows (paint it without tracers)");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const bool lds = frame_route_lds(render_px);
  if (int rc = e->frame_rgba.grow(e, (size_t)(e->n_worlds * npix) * 4)) return rc;
  if (!lds)
    if (int rc = e->frame_work.grow(e, (size_t)(e->n_worlds * npix) * 2 * sizeof(uint32_t))) return rc;
  if (rows.sizes)
    if (int rc = ens_world_table(e, rows)) return rc;
  FrameArgs a;
  a.pos = e->pos[e->cur];
  a.vel = e->vel;
  a.mass = e->mass;
  a.tpos = tracers ? rows.tpos : nullptr;
  a.tvel = tracers ? rows.tvel : nullptr;
  a.table = rows.sizes ? e->table.worlds : nullptr;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = tracers ? (uint32_t)rows.n_tracers : 0u;
  a.height = height;
  a.render_px = render_px;
  ENS_HIPCHK(e, launch_ensemble_frames<typename P::Real>(e->stream, e->n_worlds, max_rows, a, lds ? nullptr : e->frame_work.p, e->frame_rgba.p));
  ENS_HIPCHK(e, hipMemcpyAsync(rgba_out, e->frame_rgba.p, (size_t)(e->n_worlds * npix) * 4, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// ---- delta streams: every world's NBD1 stream (ensemble_deltas.h) of the current positions, into host memory
// The scratch of a sequence for its planned rows; on failure the sequence is released whole.
template <class P> int ens_deltas_scratch(EnsembleState<P>* e, DeltaSeq& q, bool tracers, const WorldRows<P>& rows) {
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
// Reads pos[cur] or the tracers.  The sequence advances only when the streams have been copied out: a refused call changes nothing.
template <class P>
int ens_deltas(EnsembleState<P>* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out, uint64_t* step_out,
               const WorldRows<P>& rows = WorldRows<P>()) {
  using K = typename std::conditional<sizeof(typename P::Real) == 8, uint64_t, uint32_t>::type;
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " deltas: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!bytes_out) return ens_fail(e, NBODY_ERR_INVALID, who + "bytes_out is NULL");
  if (!out && cap) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL with cap != 0");
  if (flags & ~(NBODY_DELTAS_TRACERS | NBODY_DELTAS_KEY)) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_DELTAS_TRACERS) != 0;
  if (tracers && !rows.has_tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_DELTAS_TRACERS on a handle without tracers");
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
  if (int rc = q.out.grow(e, total)) return rc;
  a.out = q.out.p;
  ENS_HIPCHK(e, launch_deltas_write<K>(e->stream, a));
  ENS_HIPCHK(e, hipMemcpyAsync(out, q.out.p, total, hipMemcpyDeviceToHost, e->stream));
  if (offsets_out)
    ENS_HIPCHK(e, hipMemcpyAsync(offsets_out, q.stream_off, ((size_t)e->n_worlds + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  if (step_out) *step_out = e->updates;
  q.cur = (q.cur + 1) % 3;  // the oldest keys are overwritten next time
  q.have = a.have < 2 ? a.have + 1 : 2;
  return NBODY_OK;
}

// ---- summaries: one nbody_world_summary per world (ensemble_summary.h) of the current rows, into host memory
// out: [n_worlds] records.  Reads pos[cur], vel, the masses or the tracers.  One launch for the bodies, two for the tracers where
// a world has more than 4096 of them; the only loops over worlds are the check of ref[] and, once per upload, a ragged handle's
// table.
template <class P>
int ens_summary(EnsembleState<P>* e, uint32_t flags, uint32_t height, const int32_t* ref, nbody_world_summary* out,
                const WorldRows<P>& rows = WorldRows<P>()) {
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " summary: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!out) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL");
  if (flags & ~NBODY_SUMMARY_TRACERS) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_SUMMARY_TRACERS) != 0;
  if (tracers && !rows.has_tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_SUMMARY_TRACERS on a handle without tracers");
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
    if (int rc = ens_world_table(e, rows)) return rc;
    if (tracers) n_chunks = e->table.summary_tracer_chunks;
  } else {
    n_chunks = e->n_worlds * (int64_t)summary_chunks((uint32_t)(tracers ? rows.n_tracers : e->n_bodies));
  }
  if (int rc = e->summary_out.grow(e, n * sizeof(nbody_world_summary))) return rc;
  if (n_chunks > e->n_worlds)
    if (int rc = e->summary_chunks.grow(e, (size_t)n_chunks * sizeof(nbody_world_summary))) return rc;
  if (ref) {
    if (int rc = e->summary_ref.grow(e, n * sizeof(int32_t))) return rc;
    ENS_HIPCHK(e, hipMemcpyAsync(e->summary_ref.p, ref, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  }
  SummaryArgs a;
  a.pos = e->pos[e->cur];
  a.vel = e->vel;
  a.mass = e->mass;
  a.tpos = rows.tpos;
  a.tvel = rows.tvel;
  a.table = rows.sizes ? e->table.worlds : nullptr;
  a.chunk_base = rows.sizes ? e->table.summary_chunk_base : nullptr;
  a.ref = ref ? e->summary_ref.p : nullptr;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = (uint32_t)rows.n_tracers;
  a.n_worlds = (uint32_t)e->n_worlds;
  a.height = height;
  a.tracers = tracers ? 1u : 0u;
  ENS_HIPCHK(e, launch_ensemble_summary<typename P::Real>(e->stream, a, n_chunks, e->summary_chunks.p, e->summary_out.p));
  ENS_HIPCHK(e, hipMemcpyAsync(out, e->summary_out.p, n * sizeof(nbody_world_summary), hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// ---- encounters: per target its nearest source and its clamped pairs, per world one nbody_world_encounters
// (ensemble_encounters.h) of the current rows, into host memory
// out: [n_worlds] records; nn_index, nn_d2, close: one entry per target of all worlds, each may be NULL.  Reads pos[cur] and the
// tracers' positions.  Two launches; no loop over worlds but, once per upload, a ragged handle's table.
template <class P>
int ens_encounters(EnsembleState<P>* e, uint32_t flags, const float* limit2, nbody_world_encounters* out, int32_t* nn_index,
                   typename P::Real* nn_d2, uint32_t* close, const WorldRows<P>& rows = WorldRows<P>()) {
  using Real = typename P::Real;
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " encounters: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!out) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL");
  if (flags & ~NBODY_ENCOUNTERS_TRACERS) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_ENCOUNTERS_TRACERS) != 0;
  if (tracers && !rows.has_tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_ENCOUNTERS_TRACERS on a handle without tracers");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const size_t n = (size_t)e->n_worlds;
  int64_t n_tiles;
  if (rows.sizes) {
    if (int rc = ens_world_table(e, rows)) return rc;
    n_tiles = tracers ? e->table.enc_tracer_tiles : e->table.enc_body_tiles;
  } else {
    n_tiles = e->n_worlds * (int64_t)encounter_tiles((uint32_t)(tracers ? rows.n_tracers : e->n_bodies));
  }
  const size_t t = (size_t)(tracers ? rows.tracer_rows : e->rows);  // the targets (<= 2^26)
  if (int rc = e->enc_out.grow(e, n * sizeof(nbody_world_encounters))) return rc;
  if (t) {
    if (int rc = e->enc_index.grow(e, t * sizeof(int32_t))) return rc;
    if (int rc = e->enc_d2.grow(e, t * sizeof(Real))) return rc;
    if (int rc = e->enc_close.grow(e, t * sizeof(uint32_t))) return rc;
    if (int rc = e->enc_live.grow(e, t * sizeof(uint32_t))) return rc;
  }
  if (limit2) {
    if (int rc = e->enc_limit.grow(e, n * sizeof(float))) return rc;
    ENS_HIPCHK(e, hipMemcpyAsync(e->enc_limit.p, limit2, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  }
  EncounterArgs a;
  a.pos = e->pos[e->cur];
  a.tpos = rows.tpos;
  a.table = rows.sizes ? e->table.worlds : nullptr;
  a.tile_base = rows.sizes ? e->table.enc_tile_base + (tracers ? n + 1 : 0) : nullptr;
  a.limit2 = limit2 ? e->enc_limit.p : nullptr;
  a.limit_all = e->params.clamp;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = (uint32_t)rows.n_tracers;
  a.n_worlds = (uint32_t)e->n_worlds;
  a.tracers = tracers ? 1u : 0u;
  a.nn_index = e->enc_index.p;
  a.nn_d2 = e->enc_d2.p;
  a.close = e->enc_close.p;
  a.live = e->enc_live.p;
  ENS_HIPCHK(e, launch_ensemble_encounters<Real>(e->stream, a, n_tiles, e->enc_out.p));
  ENS_HIPCHK(e, hipMemcpyAsync(out, e->enc_out.p, n * sizeof(nbody_world_encounters), hipMemcpyDeviceToHost, e->stream));
  if (t && nn_index) ENS_HIPCHK(e, hipMemcpyAsync(nn_index, e->enc_index.p, t * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (t && nn_d2) ENS_HIPCHK(e, hipMemcpyAsync(nn_d2, e->enc_d2.p, t * sizeof(Real), hipMemcpyDeviceToHost, e->stream));
  if (t && close) ENS_HIPCHK(e, hipMemcpyAsync(close, e->enc_close.p, t * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// ---- a watched run: an update whose samples — before, between and after its steps — are folded on the device into six values
// per target and one nbody_world_watch per world (ensemble_watch.h), into host memory
// The per-target outputs of the call in the handle's precision: nbody_watch_rows_f32 or nbody_watch_rows_f64.
template <class Real> struct WatchRowsOf { using type = nbody_watch_rows_f32; };
template <> struct WatchRowsOf<double> { using type = nbody_watch_rows_f64; };

// The scratch of a watched run and the two argument structs over it: the records, the six running rows per target, the call's
// limit2[] (host, [n_worlds], or NULL: params.clamp) on its way to the device.  a.pos is the caller's to set before every launch.
struct WatchScratch {
  EncounterArgs a;
  WatchRun w;
  int64_t n_tiles = 0;
  size_t targets = 0;  // of all worlds (<= 2^26)
};
template <class P>
int ens_watch_scratch(EnsembleState<P>* e, bool tracers, const float* limit2, uint32_t height, const WorldRows<P>& rows, WatchScratch& ws) {
  using Real = typename P::Real;
  const size_t n = (size_t)e->n_worlds;
  int64_t n_tiles;
  if (rows.sizes) {
    if (int rc = ens_world_table(e, rows)) return rc;
    n_tiles = tracers ? e->table.enc_tracer_tiles : e->table.enc_body_tiles;
  } else {
    n_tiles = e->n_worlds * (int64_t)encounter_tiles((uint32_t)(tracers ? rows.n_tracers : e->n_bodies));
  }
  const size_t t = (size_t)(tracers ? rows.tracer_rows : e->rows);
  if (int rc = e->watch_out.grow(e, n * sizeof(nbody_world_watch))) return rc;
  if (t) {
    if (int rc = e->watch_d2.grow(e, t * sizeof(Real))) return rc;
    if (int rc = e->watch_index.grow(e, t * sizeof(int32_t))) return rc;
    if (int rc = e->watch_sample.grow(e, t * sizeof(uint32_t))) return rc;
    if (int rc = e->watch_first_close.grow(e, t * sizeof(uint32_t))) return rc;
    if (int rc = e->watch_close_samples.grow(e, t * sizeof(uint32_t))) return rc;
    if (int rc = e->watch_first_out.grow(e, t * sizeof(uint32_t))) return rc;
  }
  if (limit2) {
    if (int rc = e->watch_limit.grow(e, n * sizeof(float))) return rc;
    ENS_HIPCHK(e, hipMemcpyAsync(e->watch_limit.p, limit2, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  }
  EncounterArgs& a = ws.a;
  a.tpos = rows.tpos;
  a.table = rows.sizes ? e->table.worlds : nullptr;
  a.tile_base = rows.sizes ? e->table.enc_tile_base + (tracers ? n + 1 : 0) : nullptr;
  a.limit2 = limit2 ? e->watch_limit.p : nullptr;
  a.limit_all = e->params.clamp;
  a.n_bodies = (uint32_t)e->n_bodies;
  a.n_tracers = (uint32_t)rows.n_tracers;
  a.n_worlds = (uint32_t)e->n_worlds;
  a.tracers = tracers ? 1u : 0u;
  WatchRun& w = ws.w;
  w.min_d2 = e->watch_d2.p;
  w.min_index = e->watch_index.p;
  w.min_sample = e->watch_sample.p;
  w.first_close = e->watch_first_close.p;
  w.close_samples = e->watch_close_samples.p;
  w.first_out = e->watch_first_out.p;
  w.height = height;
  ws.n_tiles = n_tiles;
  ws.targets = t;
  return NBODY_OK;
}

// The running rows of all t targets into the caller's arrays, each of which may be NULL (enqueued, not waited for).
template <class P> int ens_watch_copy_rows(EnsembleState<P>* e, const typename WatchRowsOf<typename P::Real>::type* out_rows, size_t t) {
  using Real = typename P::Real;
  const auto copy = [&](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
  };
  ENS_HIPCHK(e, copy(out_rows->min_d2, e->watch_d2.p, t * sizeof(Real)));
  ENS_HIPCHK(e, copy(out_rows->min_index, e->watch_index.p, t * sizeof(int32_t)));
  ENS_HIPCHK(e, copy(out_rows->min_sample, e->watch_sample.p, t * sizeof(uint32_t)));
  ENS_HIPCHK(e, copy(out_rows->first_close, e->watch_first_close.p, t * sizeof(uint32_t)));
  ENS_HIPCHK(e, copy(out_rows->close_samples, e->watch_close_samples.p, t * sizeof(uint32_t)));
  ENS_HIPCHK(e, copy(out_rows->first_out, e->watch_first_out.p, t * sizeof(uint32_t)));
  return NBODY_OK;
}

// out: [n_worlds] records; out_rows: NULL or the six arrays, each NULL or one entry per target of all worlds.  `launch(args)` as
// in ens_update_with, and the steps are enqueued as it enqueues them: the run is an update's, bit for bit.  One sampling launch
// per taken sample, one reduce at the end, one synchronise; no loop over worlds but, once per upload, a ragged handle's table.
template <class P, class Launch>
int ens_watch_with(EnsembleState<P>* e, uint32_t flags, typename P::Real delta, int n_steps, int stride, const float* limit2, uint32_t height,
                   nbody_world_watch* out, const typename WatchRowsOf<typename P::Real>::type* out_rows, nbody_counting* counter,
                   const WorldRows<P>& rows, Launch launch) {
  using Real = typename P::Real;
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " watch: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!out) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL");
  if (flags & ~(NBODY_WATCH_TRACERS | NBODY_WATCH_RESUME)) return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
  const bool tracers = (flags & NBODY_WATCH_TRACERS) != 0;
  if (tracers && !rows.has_tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_WATCH_TRACERS on a handle without tracers");
  if (n_steps < 0) return ens_fail(e, NBODY_ERR_INVALID, who + "n_steps < 0");
  if (stride < 1) return ens_fail(e, NBODY_ERR_INVALID, who + "stride must be >= 1");
  if (height > kWatchMaxHeight) return ens_fail(e, NBODY_ERR_INVALID, who + "height must be <= 2^24");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  const size_t n = (size_t)e->n_worlds;
  WatchScratch ws;
  if (int rc = ens_watch_scratch(e, tracers, limit2, height, rows, ws)) return rc;
  EncounterArgs& a = ws.a;
  WatchRun& w = ws.w;
  const int64_t n_tiles = ws.n_tiles;
  const size_t t = ws.targets;
  const int per_lane = lab_int("NBODY_WATCH_PER_LANE", kWatchPerLane);
  uint32_t samples = 0;
  for (int s = 0;; ++s) {
    if (s % stride == 0 && !(s == 0 && (flags & NBODY_WATCH_RESUME))) {
      a.pos = e->pos[e->cur];  // (the tracers are stepped in place)
      w.sample = (uint32_t)s;
      w.first = samples == 0 ? 1u : 0u;
      ENS_HIPCHK(e, launch_ensemble_watch_sample<Real>(e->stream, a, w, n_tiles, per_lane));
      ++samples;
    }
    if (s == n_steps) break;
    ENS_HIPCHK(e, ens_enqueue_step(e, delta, launch));
  }
  a.pos = e->pos[e->cur];
  ENS_HIPCHK(e, launch_ensemble_watch_worlds<Real>(e->stream, a, w, samples, e->watch_out.p));
  ENS_HIPCHK(e, hipMemcpyAsync(out, e->watch_out.p, n * sizeof(nbody_world_watch), hipMemcpyDeviceToHost, e->stream));
  if (t && out_rows && samples)
    if (int rc = ens_watch_copy_rows(e, out_rows, t)) return rc;
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  if (t && out_rows && !samples) {  // no sample was taken: the device rows were never written, every target is as it began
    if (out_rows->min_d2) std::fill(out_rows->min_d2, out_rows->min_d2 + t, std::numeric_limits<Real>::infinity());
    if (out_rows->min_index) std::fill(out_rows->min_index, out_rows->min_index + t, -1);
    if (out_rows->min_sample) std::fill(out_rows->min_sample, out_rows->min_sample + t, NBODY_WATCH_NEVER);
    if (out_rows->first_close) std::fill(out_rows->first_close, out_rows->first_close + t, NBODY_WATCH_NEVER);
    if (out_rows->close_samples) std::fill(out_rows->close_samples, out_rows->close_samples + t, 0u);
    if (out_rows->first_out) std::fill(out_rows->first_out, out_rows->first_out + t, NBODY_WATCH_NEVER);
  }
  const double dt = now_s() - t_begin;  // booked as an update's seconds are
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
}

// ---- a watched sweep: a sweep (ens_sweep_with) watched as ens_watch_with watches an update, every world on a schedule of its
// own: sample s of world k iff s <= steps[k], s % stride[k] == 0 and not (s == 0 under NBODY_WATCH_RESUME).  The steps are the
// sweep's (ens_enqueue_sweep_step over its table), the scratch is the watch's, and the schedules are one WatchWorld per world on
// the device.  One sampling launch at every s that some world takes — the host asks WatchSchedule::any, it does not walk the
// samples — one reduce, one synchronise.  limit2 NULL: world k's limit is clamp[k]; both NULL: params.clamp.
template <class P, class Launch>
int ens_wsweep_with(EnsembleState<P>* e, uint32_t flags, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps,
                    const int32_t* stride, const float* limit2, uint32_t height, nbody_world_watch* out,
                    const typename WatchRowsOf<typename P::Real>::type* out_rows, nbody_counting* counter, const WorldRows<P>& rows, Launch launch) {
  using Real = typename P::Real;
  if (!e) return NBODY_ERR_INVALID;
  const std::string who = std::string(P::kWho) + " wsweep: ";
  if (!e->n_worlds) return ens_fail(e, NBODY_ERR_INVALID, who + "nothing uploaded");
  if (!out) return ens_fail(e, NBODY_ERR_INVALID, who + "out is NULL");
  if (!delta) return ens_fail(e, NBODY_ERR_INVALID, who + "delta is NULL");
  const bool tracers = (flags & NBODY_WATCH_TRACERS) != 0;
  int64_t k = 0;
  switch (WatchSchedule::check(e->n_worlds, steps, n_steps, stride, flags, &k)) {
    case WatchSchedule::kOk: break;
    case WatchSchedule::kBadFlags: return ens_fail(e, NBODY_ERR_INVALID, who + "unknown flag bits");
    case WatchSchedule::kStepOutside:
      return ens_fail(e, NBODY_ERR_INVALID, who + "steps[" + std::to_string(k) + "] = " + std::to_string(steps[k]) + " of world " + std::to_string(k) +
                                                " is outside 0 .. n_steps = " + std::to_string(n_steps));
    case WatchSchedule::kBadStride:
      return ens_fail(e, NBODY_ERR_INVALID, who + "stride[" + std::to_string(k) + "] = " + std::to_string(stride[k]) + " of world " +
                                                std::to_string(k) + " must be >= 1");
    default: return ens_fail(e, NBODY_ERR_INVALID, who + "n_steps < 0");
  }
  if (tracers && !rows.has_tracer_calls) return ens_fail(e, NBODY_ERR_INVALID, who + "NBODY_WATCH_TRACERS on a handle without tracers");
  if (height > kWatchMaxHeight) return ens_fail(e, NBODY_ERR_INVALID, who + "height must be <= 2^24");

  ENS_HIPCHK(e, hipSetDevice(e->device));
  const double t_begin = now_s();
  const size_t n = (size_t)e->n_worlds;
  WatchScratch ws;
  if (int rc = ens_watch_scratch(e, tracers, limit2 ? limit2 : clamp, height, rows, ws)) return rc;
  e->watch_sched_host.resize(n);  // (the handle's, as the sweep's table is)
  WatchSchedule schedule;
  schedule.build(e->n_worlds, steps, n_steps, stride, flags, e->watch_sched_host.data());
  if (int rc = e->watch_sched.grow(e, n * sizeof(WatchWorld))) return rc;
  ENS_HIPCHK(e, hipMemcpyAsync(e->watch_sched.p, e->watch_sched_host.data(), n * sizeof(WatchWorld), hipMemcpyHostToDevice, e->stream));
  if (n_steps > 0)
    if (int rc = ens_sweep_table(e, delta, clamp, steps, n_steps)) return rc;
  for (int s = 0;; ++s) {
    if (schedule.any(s)) {
      ws.a.pos = e->pos[e->cur];  // (the tracers are stepped in place)
      ws.w.sample = (uint32_t)s;
      ENS_HIPCHK(e, launch_ensemble_watch_sample<Real>(e->stream, ws.a, ws.w, ws.n_tiles, kWatchPerLane, e->watch_sched.p));
    }
    if (s == n_steps) break;
    ENS_HIPCHK(e, ens_enqueue_sweep_step(e, clamp != nullptr, s, launch));
  }
  ws.a.pos = e->pos[e->cur];
  ENS_HIPCHK(e, launch_ensemble_watch_worlds<Real>(e->stream, ws.a, ws.w, 0u, e->watch_out.p, e->watch_sched.p));
  ENS_HIPCHK(e, hipMemcpyAsync(out, e->watch_out.p, n * sizeof(nbody_world_watch), hipMemcpyDeviceToHost, e->stream));
  if (ws.targets && out_rows)  // (the reduce has written the rows of the worlds that took no sample)
    if (int rc = ens_watch_copy_rows(e, out_rows, ws.targets)) return rc;
  ENS_HIPCHK(e, hipStreamSynchronize(e->stream));
  const double dt = now_s() - t_begin;  // booked as an update's seconds are
  e->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  return NBODY_OK;
}

// The schedules of a watched sweep as the ABI shows them (nbody_wsweep_plan): pure host code, the call's own refusals, no message.
inline int wsweep_show_plan(int64_t n_worlds, const int32_t* steps, int n_steps, const int32_t* stride, uint32_t flags, int64_t* samples_of_world,
                            int64_t* n_sampling_launches) {
  int64_t k = 0;
  if (WatchSchedule::check(n_worlds, steps, n_steps, stride, flags, &k) != WatchSchedule::kOk) return NBODY_ERR_INVALID;
  WatchSchedule schedule;
  schedule.build(n_worlds, steps, n_steps, stride, flags, nullptr);
  if (samples_of_world)
    for (k = 0; k < n_worlds; ++k)
      samples_of_world[k] = WatchSchedule::world(steps ? steps[k] : n_steps, stride ? stride[k] : 1, schedule.resume).samples;
  if (n_sampling_launches) {
    int64_t launches = 0;
    for (int s = 0;; ++s) {
      launches += schedule.any(s) ? 1 : 0;
      if (s == n_steps) break;
    }
    *n_sampling_launches = launches;
  }
  return NBODY_OK;
}

#undef ENS_HIPCHK

}  // namespace nbody
