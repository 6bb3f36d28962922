// Ragged ensembles (nbody_ragged_*, nbody_ragged64_*): the launch plan of worlds of different sizes.  Internal, host only, plain
// C++ (no HIP include): nbody_ragged_plan / nbody_ragged64_plan, the handles' upload and the stand-alone check of
// tools/ragged_plan_check.cpp use this one header.  The plan is written over the precision's LDS function: ensemble_lds_bytes
// (f32, the default) or ensemble64_lds_bytes; classes, tiles and work items are the same in both.
//
// Launch classes.  Worlds are grouped by the LDS they need, in size order: n <= 128, <= 256, <= 512, <= 1024, <= 2048, <= 4096.
//   Every class that has a world is one launch per step (at most kRaggedMaxLaunches), in class order; its dynamic LDS is
//   the LDS function of its LARGEST member, not of the class cap: equal sizes get exactly the uniform ensemble's LDS, and no
//   world above 128 bodies sits under more than twice its own need.  The first class holds every lane split (ensemble_split:
//   2 .. 64 lanes per target) under at most 1.5 KB (f32; 2.5 KB in f64).  The class caps in f64: 2 560, 5 120, 10 240, 20 480,
//   40 960 and 81 920 B.  The boundaries are the six doublings in both precisions: reasoned, not measured.
// Work items.  Within a launch a block is one (world, tile) item; a world's blocks are contiguous, tile ascending, and the
//   worlds of a launch follow one another in world order.  tiles = ceil(n / (256 / ensemble_split(n))), as in the uniform launch.
//   The device table holds one 8-byte item per block, {row0, n | tile << 16}: row0 < 2^26, n <= 4096, tile <= 15.
#pragma once
#include <stdint.h>

#include "ensemble_shape.h"

namespace nbody {

constexpr int kRaggedMaxLaunches = 6;

struct RaggedItem {  // the layout of the device's uint2
  uint32_t row0;
  uint32_t n_tile;   // n | tile << 16
};
static_assert(sizeof(RaggedItem) == 8, "one work item is 8 bytes");

// The launch class of a world: 0 for n <= 128, then one per doubling up to 4096.
inline int ragged_class(int64_t n_bodies) {
  int cls = 0;
  for (int64_t cap = 128; cap < n_bodies; cap *= 2) ++cls;
  return cls;
}
inline int ragged_tiles(int n_bodies) {
  const int tpb = kEnsembleBlock / ensemble_split(n_bodies);
  return (n_bodies + tpb - 1) / tpb;
}

struct RaggedPlan {
  int32_t n_launches = 0;
  int32_t lds_bytes[kRaggedMaxLaunches] = {};  // per launch
  int64_t blocks[kRaggedMaxLaunches] = {};     // per launch
  int64_t rows = 0;                            // sum of the sizes
  int64_t total_blocks = 0;
  int32_t launch_of_class[kRaggedMaxLaunches] = {-1, -1, -1, -1, -1, -1};
};

enum { kRaggedOk = 0, kRaggedNoWorld = 1, kRaggedBadSize = 2, kRaggedTooManyRows = 3 };

typedef size_t (*RaggedLdsFn)(int n_bodies);  // the dynamic LDS of a world of n_bodies: ensemble_lds_bytes or ensemble64_lds_bytes

// The plan of `n_worlds` worlds of the sizes n_bodies[]: per launch its LDS and its blocks; per world (either array may be NULL)
// its launch and the first of its blocks in that launch.  Nothing is written unless the sizes are valid.
inline int ragged_plan(int64_t n_worlds, const int64_t* n_bodies, RaggedPlan* plan, int32_t* launch_of_world, int64_t* first_block_of_world,
                       RaggedLdsFn lds_bytes_of = ensemble_lds_bytes) {
  if (n_worlds < 1 || !n_bodies) return kRaggedNoWorld;
  if (n_worlds > kEnsembleMaxRows) return kRaggedTooManyRows;  // (every world has a row)
  RaggedPlan p;
  int max_n[kRaggedMaxLaunches] = {};
  int64_t class_blocks[kRaggedMaxLaunches] = {};
  for (int64_t k = 0; k < n_worlds; ++k) {
    const int64_t n = n_bodies[k];
    if (n < 1 || n > kEnsembleMaxBodies) return kRaggedBadSize;
    p.rows += n;
    if (p.rows > kEnsembleMaxRows) return kRaggedTooManyRows;
    const int cls = ragged_class(n);
    if ((int)n > max_n[cls]) max_n[cls] = (int)n;
    class_blocks[cls] += ragged_tiles((int)n);
  }
  for (int cls = 0; cls < kRaggedMaxLaunches; ++cls) {
    if (!max_n[cls]) continue;  // an empty class launches nothing
    p.launch_of_class[cls] = p.n_launches;
    p.lds_bytes[p.n_launches] = (int32_t)lds_bytes_of(max_n[cls]);
    p.blocks[p.n_launches] = class_blocks[cls];
    p.total_blocks += class_blocks[cls];
    ++p.n_launches;
  }
  if (launch_of_world || first_block_of_world) {
    int64_t next[kRaggedMaxLaunches] = {};
    for (int64_t k = 0; k < n_worlds; ++k) {
      const int l = p.launch_of_class[ragged_class(n_bodies[k])];
      if (launch_of_world) launch_of_world[k] = l;
      if (first_block_of_world) first_block_of_world[k] = next[l];
      next[l] += ragged_tiles((int)n_bodies[k]);
    }
  }
  if (plan) *plan = p;
  return kRaggedOk;
}

// The work items of a valid plan, launch after launch: launch l's items are items[first_item[l] .. first_item[l] + blocks[l]).
// `items` has plan.total_blocks elements, `first_item` kRaggedMaxLaunches.  An item's layout has no room for its world: where
// `world_of_item` is given (plan.total_blocks elements) it receives the world of every item, in the items' order.
inline void ragged_items(int64_t n_worlds, const int64_t* n_bodies, const RaggedPlan& plan, RaggedItem* items, int64_t* first_item,
                         uint32_t* world_of_item = nullptr) {
  int64_t next[kRaggedMaxLaunches] = {}, at = 0;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) {
    first_item[l] = next[l] = l < plan.n_launches ? at : 0;
    if (l < plan.n_launches) at += plan.blocks[l];
  }
  int64_t row0 = 0;
  for (int64_t k = 0; k < n_worlds; ++k) {
    const int n = (int)n_bodies[k];
    const int l = plan.launch_of_class[ragged_class(n)];
    const int tiles = ragged_tiles(n);
    for (int t = 0; t < tiles; ++t) {
      if (world_of_item) world_of_item[next[l]] = (uint32_t)k;
      items[next[l]++] = RaggedItem{(uint32_t)row0, (uint32_t)n | ((uint32_t)t << 16)};
    }
    row0 += n;
  }
}

}  // namespace nbody
