// libnbody_hip — ragged restricted ensembles: the host driver behind nbody_rr_* (rr.hip), written over a precision P as the
// drivers it is composed of are, so that a double-precision sibling needs a policy struct and its kernel only.  Internal.
// The bodies are the ragged ensemble's, whole: RaggedState<P> with its plan and work items, ragged_upload, ragged_launch_all,
// and through them the ensemble's state, create / destroy, params, errors, download and the *_with functions.  The tracers are
// restricted_driver.h's half, restated for rows that are not m per world: beside the bodies the handle keeps the tracer rows of
// all worlds one after another, their counts, the tracers' plan of rr_plan.h and its work-item table.  A step is the bodies'
// launches (at most 6) and then the tracers' (at most 6), all given the same P::Args: the tracers read the buffer the bodies'
// launches read (pos_in, the pre-step positions — the bodies write the other buffer), and the next step's launches follow in
// stream order.  Nothing is read back and nothing waits between the steps of a call.
//
// P supplies what ragged_driver.h asks for (kWho "ragged restricted") and, for the tracers:
//   Tracers                                                          the tracer kernel's arguments (tpos, tvel, tacc_out);
//   launch_tracer_items(stream, blocks, lds_bytes, items, args, t)   one launch of the tracers' plan: `blocks` items from `items`.
#pragma once
#include "ragged_driver.h"
#include "rr_plan.h"

namespace nbody {

template <class P> struct RrState : RaggedState<P> {
  std::vector<int64_t> counts;  // tracers per world; empty: none
  RrPlan tplan;
  int64_t tfirst_item[kRaggedMaxLaunches] = {};
  uint4* titems = nullptr;      // the tracers' work items on the device, launch after launch
  uint32_t* titem_world = nullptr;  // beside them, the world of every item (a sweep's launches read it)
  int64_t tracer_rows = 0;      // 0: no tracers
  typename P::Vec2* tpos = nullptr;
  typename P::Vec2* tvel = nullptr;
  typename P::Vec2* tacc = nullptr;
  ~RrState() { drop_tracers(); }  // (ens_destroy has made the device current and drained the stream)
  void drop_tracers() {
    free_dev(tpos); free_dev(tvel); free_dev(tacc); free_dev(titems); free_dev(titem_world);
    counts.clear();
    tplan = RrPlan();
    tracer_rows = 0;
    this->table.invalidate();  // (the table of row ranges holds the counts)
    this->dtracers.release();  // (the tracers' delta streams start over with the next tracers)
  }
};

template <class P> int rr_fail(RrState<P>* e, const char* msg) { return ens_fail<P>(e, NBODY_ERR_INVALID, msg); }
#define RR_HIPCHK(e, call)                                         \
  do {                                                             \
    hipError_t h__ = (call);                                       \
    if (h__ != hipSuccess) return ens_fail_hip<P>(e, h__, #call);  \
  } while (0)

// The message of sizes or counts that rr_plan refused (for the sizes alone: ragged_plan's codes).
inline const char* rr_plan_error(int rc) {
  switch (rc) {
    case kRaggedNoWorld: return "ragged restricted: n_worlds must be >= 1 and n_bodies not NULL";
    case kRaggedBadSize: return "ragged restricted: every world's n_bodies must be 1 .. 4096 (above that a context per world is the tool)";
    case kRaggedTooManyRows: return "ragged restricted: the sizes must add up to at most 2^26 rows";
    case kRrNoCounts: return "ragged restricted: n_tracers is NULL";
    case kRrBadCount: return "ragged restricted: every world's n_tracers must be >= 0";
    default: return "ragged restricted: the tracers must add up to at most 2^26 rows";
  }
}

// Every launch of the tracers' plan, in order.
template <class P> hipError_t rr_launch_tracers(const RrState<P>* e, const typename P::Args& a, const typename P::Tracers& t) {
  typename P::Args b = a;
  for (int l = 0; l < e->tplan.n_launches; ++l) {
    b.item_world = e->titem_world + e->tfirst_item[l];
    const hipError_t h = P::launch_tracer_items(e->stream, e->tplan.blocks[l], (size_t)e->tplan.lds_bytes[l], e->titems + e->tfirst_item[l], b, t);
    if (h != hipSuccess) return h;
  }
  return hipSuccess;
}

// The ragged upload with the tracers' fate added.  Refused for its arguments, it leaves bodies and tracers as they were; past the
// check the tracers go, with the bodies where the store fails and as those of new worlds where it succeeds.
template <class P>
int rr_upload(RrState<P>* e, int64_t n_worlds, const int64_t* n_bodies, const typename P::Real* pos, const typename P::Real* vel,
              const uint32_t* weight) {
  if (!e) return NBODY_ERR_INVALID;
  if (const int rc = ragged_plan(n_worlds, n_bodies, nullptr, nullptr, nullptr, P::lds_bytes)) return rr_fail(e, rr_plan_error(rc));
  if (!pos || !vel) return rr_fail(e, "ragged restricted upload: pos_xy or vel_xy is NULL");
  const int rc = ragged_upload<P>(e, n_worlds, n_bodies, pos, vel, weight);  // (drains the stream before it frees)
  e->drop_tracers();
  return rc;
}

template <class P>
int rr_tracers_upload(RrState<P>* e, int64_t n_worlds, const int64_t* n_tracers, const typename P::Real* pos, const typename P::Real* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rr_fail(e, "ragged restricted tracers_upload: nothing uploaded (the bodies come first)");
  if (n_worlds != e->n_worlds) return rr_fail(e, "ragged restricted tracers_upload: n_worlds is not the number of worlds of the bodies");
  RrPlan plan;
  if (const int rc = rr_plan(n_worlds, e->sizes.data(), n_tracers, &plan, nullptr, nullptr, P::lds_bytes)) return rr_fail(e, rr_plan_error(rc));
  if (plan.tracer_rows > 0 && (!pos || !vel)) return rr_fail(e, "ragged restricted tracers_upload: pos_xy or vel_xy is NULL");
  RR_HIPCHK(e, hipSetDevice(e->device));
  RR_HIPCHK(e, hipStreamSynchronize(e->stream));
  e->drop_tracers();
  if (plan.tracer_rows == 0) return NBODY_OK;
  std::vector<RrItem> items((size_t)plan.total_blocks);
  std::vector<uint32_t> item_world(items.size());
  int64_t first_item[kRaggedMaxLaunches];
  rr_items(n_worlds, e->sizes.data(), n_tracers, plan, items.data(), first_item, item_world.data());
  const size_t bytes = (size_t)plan.tracer_rows * sizeof(typename P::Vec2);
  hipError_t h = hipMalloc((void**)&e->tpos, bytes);
  if (h == hipSuccess) h = hipMalloc((void**)&e->tvel, bytes);
  if (h == hipSuccess) h = hipMalloc((void**)&e->titems, items.size() * sizeof(RrItem));
  if (h == hipSuccess) h = hipMalloc((void**)&e->titem_world, item_world.size() * sizeof(uint32_t));
  if (h == hipSuccess) h = hipMemcpyAsync(e->tpos, pos, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tvel, vel, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->titems, items.data(), items.size() * sizeof(RrItem), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->titem_world, item_world.data(), item_world.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    e->drop_tracers();
    return ens_fail_hip<P>(e, h, "upload of the tracers");
  }
  e->counts.assign(n_tracers, n_tracers + n_worlds);
  e->tplan = plan;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) e->tfirst_item[l] = first_item[l];
  e->tracer_rows = plan.tracer_rows;
  return NBODY_OK;
}

template <class P> int rr_tracers_download(RrState<P>* e, typename P::Real* pos, typename P::Real* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rr_fail(e, "ragged restricted tracers_download: nothing uploaded");
  if (!e->tracer_rows) return NBODY_OK;
  RR_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)e->tracer_rows * sizeof(typename P::Vec2);
  if (pos) RR_HIPCHK(e, hipMemcpyAsync(pos, e->tpos, bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) RR_HIPCHK(e, hipMemcpyAsync(vel, e->tvel, bytes, hipMemcpyDeviceToHost, e->stream));
  RR_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// One step: the bodies' launches and then the tracers', all given `a`.
template <class P> hipError_t rr_launch_step(RrState<P>* e, const typename P::Args& a) {
  const hipError_t h = ragged_launch_all<P>(e, a);
  if (h != hipSuccess || !e->tracer_rows) return h;
  typename P::Tracers t;
  t.tpos = e->tpos;
  t.tvel = e->tvel;
  return rr_launch_tracers<P>(e, a, t);  // a.pos_in: what the bodies' launches above read
}

template <class P> int rr_update(RrState<P>* e, typename P::Real delta, int n_steps, nbody_counting* counter) {
  return ens_update_with<P>(e, delta, n_steps, counter, [e](const typename P::Args& a) { return rr_launch_step<P>(e, a); });
}

// A sweep: the tracers of world k follow its delta, clamp and steps (every launch reads the same table).
template <class P>
int rr_sweep(RrState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter) {
  return ens_sweep_with<P>(e, delta, clamp, steps, n_steps, counter, [e](const typename P::Args& a) { return rr_launch_step<P>(e, a); });
}

template <class P> int rr_accel(RrState<P>* e, typename P::Real* acc_xy) { return ragged_accel<P>(e, acc_xy); }

template <class P> int rr_tracers_accel(RrState<P>* e, typename P::Real* acc_xy) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rr_fail(e, "ragged restricted tracers_accel: nothing uploaded");
  if (!e->tracer_rows) return NBODY_OK;
  if (!acc_xy) return rr_fail(e, "ragged restricted tracers_accel: acc_xy is NULL");
  RR_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)e->tracer_rows * sizeof(typename P::Vec2);
  if (!e->tacc) RR_HIPCHK(e, hipMalloc((void**)&e->tacc, bytes));
  typename P::Tracers t;
  t.tpos = e->tpos;
  t.tacc_out = e->tacc;
  RR_HIPCHK(e, rr_launch_tracers<P>(e, ens_args<P>(e), t));
  RR_HIPCHK(e, hipMemcpyAsync(acc_xy, e->tacc, bytes, hipMemcpyDeviceToHost, e->stream));
  RR_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// Where the handle's rows are, for the observers (ensemble_observers.h); of no handle, nothing (they refuse it).  The counts go
// with the tracers; a world without tracers is painted from its bodies, its tracer stream a header of 0 rows and its tracer
// records of rows == 0.
template <class P> WorldRows<P> rr_rows(const RrState<P>* e) {
  WorldRows<P> rows;
  rows.has_tracer_calls = true;
  if (!e) return rows;
  rows.sizes = e->sizes.data();
  if (e->tracer_rows) rows.counts = e->counts.data();
  rows.tracer_rows = e->tracer_rows;
  rows.tpos = e->tpos;
  rows.tvel = e->tvel;
  return rows;
}

// The sizes and the tracer counts of every world; either output may be NULL.  Without tracers every count is 0.
template <class P> int rr_sizes(const RrState<P>* e, int64_t* n_bodies_out, int64_t* n_tracers_out) {
  if (!e) return NBODY_ERR_INVALID;
  for (int64_t k = 0; k < e->n_worlds; ++k) {
    if (n_bodies_out) n_bodies_out[k] = e->sizes[(size_t)k];
    if (n_tracers_out) n_tracers_out[k] = e->counts.empty() ? 0 : e->counts[(size_t)k];
  }
  return NBODY_OK;
}

// The tracers' plan as the ABI shows it (nbody_rr_plan): pure host code; a refusal goes to P's create-error slot.
template <class P>
int rr_show_plan(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, int32_t* launch_of_world, int64_t* first_block_of_world,
                 int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch) {
  RrPlan plan;
  if (const int rc = rr_plan(n_worlds, n_bodies, n_tracers, &plan, launch_of_world, first_block_of_world, P::lds_bytes))
    return ens_fail<P>(nullptr, NBODY_ERR_INVALID, rr_plan_error(rc));
  if (n_launches) *n_launches = plan.n_launches;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) {
    if (lds_bytes_of_launch) lds_bytes_of_launch[l] = plan.lds_bytes[l];
    if (blocks_of_launch) blocks_of_launch[l] = plan.blocks[l];
  }
  return NBODY_OK;
}

#undef RR_HIPCHK

}  // namespace nbody
