// Ragged restricted ensembles (nbody_rr_*): the launch plan of the tracers of worlds that differ in size and in their number of
// tracers.  Internal, host only, plain C++ (no HIP include): nbody_rr_plan, the handle's tracer upload and the stand-alone check
// of tools/rr_plan_check.cpp use this one header.  The bodies' plan is ragged_plan.h's, unchanged; this is the tracers'.
//
// Launch classes.  A tracer block stages its world's bodies whole in LDS as a body block does, so tracer blocks are grouped by
//   the LDS their world needs: the six classes of ragged_class(n_bodies[k]).  A class launches only if one of its worlds has
//   tracers, and its dynamic LDS is the LDS function of the largest n among the worlds of that class THAT HAVE TRACERS.  At most
//   kRaggedMaxLaunches launches, in class order.
// Work items.  World k contributes ceil(m_k / kRrTile) blocks, kRrTile = 512 tracers (256 lanes x 2 tracers per lane), their
//   tracer_row0 and count ascending: full tiles, then the rest.  A world's blocks are contiguous, and the worlds of a launch
//   follow one another in world order.  A world with m_k == 0 contributes nothing and has no launch (-1) and no block (-1).
// Tracer rows are laid out like body rows: world after world, no padding; world k's tracers are the rows [toff_k, toff_k + m_k).
//   The device table holds one 16-byte item per block, {body_row0, n, tracer_row0, count}: rows < 2^26, n <= 4096, count <= 512.
#pragma once
#include <stdint.h>

#include "ragged_plan.h"

namespace nbody {

constexpr int kRrTile = 512;  // tracers per block: kEnsembleBlock * kRestrictedPerLane (rr.hip asserts it)

struct RrItem {  // the layout of the device's uint4
  uint32_t body_row0;
  uint32_t n;
  uint32_t tracer_row0;
  uint32_t count;  // 1 .. kRrTile
};
static_assert(sizeof(RrItem) == 16, "one work item is 16 bytes");

struct RrPlan {
  int32_t n_launches = 0;
  int32_t lds_bytes[kRaggedMaxLaunches] = {};  // per launch
  int64_t blocks[kRaggedMaxLaunches] = {};     // per launch
  int64_t body_rows = 0;                       // sum of the sizes
  int64_t tracer_rows = 0;                     // sum of the tracer counts
  int64_t total_blocks = 0;
  int32_t launch_of_class[kRaggedMaxLaunches] = {-1, -1, -1, -1, -1, -1};
};

// (continuing ragged_plan.h's codes)
enum { kRrNoCounts = 4, kRrBadCount = 5, kRrTooManyTracers = 6 };

inline int64_t rr_tiles(int64_t n_tracers) { return (n_tracers + kRrTile - 1) / kRrTile; }

// The tracers' plan of `n_worlds` worlds of n_bodies[] bodies and n_tracers[] tracers: per launch its LDS and its blocks; per
// world (either array may be NULL) its launch and the first of its blocks in that launch, both -1 for a world without tracers.
// Nothing is written unless sizes and counts are valid.
inline int rr_plan(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, RrPlan* plan, int32_t* launch_of_world,
                   int64_t* first_block_of_world, RaggedLdsFn lds_bytes_of = ensemble_lds_bytes) {
  if (n_worlds < 1 || !n_bodies) return kRaggedNoWorld;
  if (!n_tracers) return kRrNoCounts;
  if (n_worlds > kEnsembleMaxRows) return kRaggedTooManyRows;  // (every world has a row)
  RrPlan p;
  int max_n[kRaggedMaxLaunches] = {};
  int64_t class_blocks[kRaggedMaxLaunches] = {};
  for (int64_t k = 0; k < n_worlds; ++k) {
    const int64_t n = n_bodies[k], m = n_tracers[k];
    if (n < 1 || n > kEnsembleMaxBodies) return kRaggedBadSize;
    p.body_rows += n;
    if (p.body_rows > kEnsembleMaxRows) return kRaggedTooManyRows;
    if (m < 0) return kRrBadCount;
    if (m > kEnsembleMaxRows - p.tracer_rows) return kRrTooManyTracers;  // (no overflow: both sides are <= 2^26)
    p.tracer_rows += m;
    if (!m) continue;
    const int cls = ragged_class(n);
    if ((int)n > max_n[cls]) max_n[cls] = (int)n;
    class_blocks[cls] += rr_tiles(m);
  }
  for (int cls = 0; cls < kRaggedMaxLaunches; ++cls) {
    if (!max_n[cls]) continue;  // a class without tracers launches nothing
    p.launch_of_class[cls] = p.n_launches;
    p.lds_bytes[p.n_launches] = (int32_t)lds_bytes_of(max_n[cls]);
    p.blocks[p.n_launches] = class_blocks[cls];
    p.total_blocks += class_blocks[cls];
    ++p.n_launches;
  }
  if (launch_of_world || first_block_of_world) {
    int64_t next[kRaggedMaxLaunches] = {};
    for (int64_t k = 0; k < n_worlds; ++k) {
      const int l = n_tracers[k] ? p.launch_of_class[ragged_class(n_bodies[k])] : -1;
      if (launch_of_world) launch_of_world[k] = l;
      if (first_block_of_world) first_block_of_world[k] = l < 0 ? -1 : next[l];
      if (l >= 0) next[l] += rr_tiles(n_tracers[k]);
    }
  }
  if (plan) *plan = p;
  return kRaggedOk;
}

// The work items of a valid plan, launch after launch: launch l's items are items[first_item[l] .. first_item[l] + blocks[l]).
// `items` has plan.total_blocks elements, `first_item` kRaggedMaxLaunches; `world_of_item`, where given, receives the world of
// every item in the items' order, as ragged_items' does.
inline void rr_items(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, const RrPlan& plan, RrItem* items,
                     int64_t* first_item, uint32_t* world_of_item = nullptr) {
  int64_t next[kRaggedMaxLaunches] = {}, at = 0;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) {
    first_item[l] = next[l] = l < plan.n_launches ? at : 0;
    if (l < plan.n_launches) at += plan.blocks[l];
  }
  int64_t body_row0 = 0, tracer_row0 = 0;
  for (int64_t k = 0; k < n_worlds; ++k) {
    const int64_t n = n_bodies[k], m = n_tracers[k];
    if (m) {
      const int l = plan.launch_of_class[ragged_class(n)];
      for (int64_t done = 0; done < m; done += kRrTile) {
        const int64_t count = m - done < kRrTile ? m - done : kRrTile;
        if (world_of_item) world_of_item[next[l]] = (uint32_t)k;
        items[next[l]++] = RrItem{(uint32_t)body_row0, (uint32_t)n, (uint32_t)(tracer_row0 + done), (uint32_t)count};
      }
    }
    body_row0 += n;
    tracer_row0 += m;
  }
}

}  // namespace nbody
