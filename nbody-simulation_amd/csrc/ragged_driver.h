// libnbody_hip — ragged ensembles: the host driver behind nbody_ragged_* (ragged.hip) and nbody_ragged64_* (ragged64.hip), written once over a precision P as
// ensemble_driver.h is, and out of its parts: the state with its double-buffered positions, in-place velocities and lazily
// allocated accelerations, create / destroy, params and errors are the ensemble's.  Internal.  What differs: the worlds have
// sizes of their own, so an upload keeps the sizes, lays out the plan of ragged_plan.h and uploads its work-item table, and one
// step is one launch per launch of that plan, back to back on the handle's stream, with one synchronise at the end of a call.
//
// P supplies what ensemble_driver.h asks for (kWho "ragged") and, in place of launch:
//   launch_items(stream, blocks, lds_bytes, items, args)   one launch of the plan: `blocks` work items from `items`;
//   lds_bytes(n_bodies)                                    the dynamic LDS of a world, which the plan sizes its launches by.
#pragma once
#include "ensemble_driver.h"
#include "ragged_plan.h"

namespace nbody {

template <class P> struct RaggedState : EnsembleState<P> {
  std::vector<int64_t> sizes;                 // per world
  RaggedPlan plan;
  int64_t first_item[kRaggedMaxLaunches] = {};
  uint2* items = nullptr;                     // the plan's work items on the device, launch after launch
  uint32_t* item_world = nullptr;             // beside them, the world of every item (a sweep's launches read it)
  ~RaggedState() { free_dev(items); free_dev(item_world); }  // (ens_destroy has made the device current and drained the stream)
};

// Every launch of the plan, in order.
template <class P> hipError_t ragged_launch_all(const RaggedState<P>* e, const typename P::Args& a) {
  typename P::Args b = a;
  for (int l = 0; l < e->plan.n_launches; ++l) {
    b.item_world = e->item_world + e->first_item[l];
    const hipError_t h = P::launch_items(e->stream, e->plan.blocks[l], (size_t)e->plan.lds_bytes[l], e->items + e->first_item[l], b);
    if (h != hipSuccess) return h;
  }
  return hipSuccess;
}

// The message of a plan that ragged_plan refused.
inline const char* ragged_plan_error(int rc) {
  switch (rc) {
    case kRaggedNoWorld: return "ragged: n_worlds must be >= 1 and n_bodies not NULL";
    case kRaggedBadSize: return "ragged: every world's n_bodies must be 1 .. 4096 (above that a context per world is the tool)";
    default: return "ragged: the sizes must add up to at most 2^26 rows";
  }
}

template <class P>
int ragged_upload(RaggedState<P>* e, int64_t n_worlds, const int64_t* n_bodies, const typename P::Real* pos, const typename P::Real* vel,
                  const uint32_t* weight) {
  if (!e) return NBODY_ERR_INVALID;
  RaggedPlan plan;
  if (const int rc = ragged_plan(n_worlds, n_bodies, &plan, nullptr, nullptr, P::lds_bytes)) return ens_fail<P>(e, NBODY_ERR_INVALID, ragged_plan_error(rc));
  if (!pos || !vel) return ens_fail<P>(e, NBODY_ERR_INVALID, "ragged upload: pos_xy or vel_xy is NULL");
  std::vector<RaggedItem> items((size_t)plan.total_blocks);
  std::vector<uint32_t> item_world(items.size());
  int64_t first_item[kRaggedMaxLaunches];
  ragged_items(n_worlds, n_bodies, plan, items.data(), first_item, item_world.data());
  if (const int rc = ens_store_rows<P>(e, plan.rows, pos, vel, weight)) return rc;  // (frees the previous arrays first)
  free_dev(e->items);
  free_dev(e->item_world);
  hipError_t h = hipMalloc((void**)&e->items, items.size() * sizeof(RaggedItem));
  if (h == hipSuccess) h = hipMalloc((void**)&e->item_world, item_world.size() * sizeof(uint32_t));
  if (h == hipSuccess) h = hipMemcpyAsync(e->items, items.data(), items.size() * sizeof(RaggedItem), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->item_world, item_world.data(), item_world.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    ens_free<P>(e);
    free_dev(e->items);
    free_dev(e->item_world);
    return ens_fail_hip<P>(e, h, "upload of the work items");
  }
  e->sizes.assign(n_bodies, n_bodies + n_worlds);
  e->plan = plan;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) e->first_item[l] = first_item[l];
  e->n_worlds = n_worlds;
  return NBODY_OK;
}

template <class P> int ragged_update(RaggedState<P>* e, typename P::Real delta, int n_steps, nbody_counting* counter) {
  return ens_update_with<P>(e, delta, n_steps, counter, [e](const typename P::Args& a) { return ragged_launch_all<P>(e, a); });
}
template <class P>
int ragged_sweep(RaggedState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter) {
  return ens_sweep_with<P>(e, delta, clamp, steps, n_steps, counter, [e](const typename P::Args& a) { return ragged_launch_all<P>(e, a); });
}
template <class P>
int ragged_resident(RaggedState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter) {
  return ens_resident_with<P>(e, delta, clamp, steps, n_steps, counter, e && e->n_worlds ? e->sizes.data() : nullptr);
}
template <class P> int ragged_accel(RaggedState<P>* e, typename P::Real* acc_xy) {
  return ens_accel_with<P>(e, acc_xy, [e](const typename P::Args& a) { return ragged_launch_all<P>(e, a); });
}

// Where the handle's rows are, for the observers (ensemble_observers.h); of no handle, nothing (they refuse it).
template <class P> WorldRows<P> ragged_rows(const RaggedState<P>* e) {
  WorldRows<P> rows;
  if (e) rows.sizes = e->sizes.data();
  return rows;
}

template <class P> int ragged_sizes(const RaggedState<P>* e, int64_t* n_bodies_out) {
  if (!e || !n_bodies_out) return NBODY_ERR_INVALID;
  for (int64_t k = 0; k < e->n_worlds; ++k) n_bodies_out[k] = e->sizes[(size_t)k];
  return NBODY_OK;
}

// The plan as the ABI shows it (nbody_ragged_plan, nbody_ragged64_plan): pure host code; a refusal goes to P's create-error slot.
template <class P>
int ragged_show_plan(int64_t n_worlds, const int64_t* n_bodies, int32_t* launch_of_world, int64_t* first_block_of_world, int32_t* n_launches,
                     int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch) {
  RaggedPlan plan;
  if (const int rc = ragged_plan(n_worlds, n_bodies, &plan, launch_of_world, first_block_of_world, P::lds_bytes))
    return ens_fail<P>(nullptr, NBODY_ERR_INVALID, ragged_plan_error(rc));
  if (n_launches) *n_launches = plan.n_launches;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) {
    if (lds_bytes_of_launch) lds_bytes_of_launch[l] = plan.lds_bytes[l];
    if (blocks_of_launch) blocks_of_launch[l] = plan.blocks[l];
  }
  return NBODY_OK;
}

}  // namespace nbody
