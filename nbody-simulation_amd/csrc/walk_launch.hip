// The one-pass walk's launch (host only): read the knobs, choose the route (walk_route.h), hand it to the launcher of the chosen
// arm (walk_arms.h).  The product and the laboratory build run this same code: lab_int gives the product the defaults, so the
// product's choice is the laboratory's choice with nothing set.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "walk_arms.h"
#include "walk_route.h"
#include "walk_split.h"

namespace nbody {

template <class T>
hipError_t launch_tree_walk_tile_main(hipStream_t s, const WalkArgs<T>& a_in, char* scratch, const WalkSplitLayout& L, const uint32_t* tgt_ids,
                                      uint32_t* hist, int64_t grid_waves, TileRoute* route) {
  TileRoute route_here;
  TileRoute& rt = route ? *route : route_here;
  rt = TileRoute{};
  if (a_in.n_tgt <= 0 || grid_waves <= 0) return hipSuccess;
  const uint32_t* off = (const uint32_t*)(scratch + L.off);
  int* info = (int*)(scratch + L.info);
  const dim3 grid((unsigned)((grid_waves + 3) / 4));
  TileLaunch k{s, grid, off, info, tgt_ids, hist, (unsigned long long*)(info + 6)};
  const TileKnobs knobs = tile_knobs_from_env();
  WalkArgs<T> a = a_in;
  a.block_stride = 1;
  a.group_order = nullptr;
  a.order_chunk = 0;
  // laboratory: more waves than the chip holds at once (256 CUs x 32): chunks of work-groups, heaviest first (walk_order_chunks)
  if constexpr (kLabBuild) {
    const int order_mode = lab_int("NBODY_WALK_ORDER", 0);  // laboratory: 2 every chunk heaviest first, 1 the lightest chunks last
    if (grid_waves > 10240 && order_mode != 0 && !knobs.wave_log && !knobs.bfs) {
      const ChunkOrder o = launch_walk_order_chunks(s, off, (int)a_in.n_tgt, info, grid.x, (int*)(scratch + L.order), order_mode);
      a.group_order = o.order;
      a.order_chunk = o.chunk;
      k.grid = dim3(o.groups);
    }
  }
  // laboratory: NBODY_WALK_BLOCK_STRIDE=1 deals the work-groups out with a golden-ratio stride (coprime with the grid) instead of in order
  if (lab_int("NBODY_WALK_BLOCK_STRIDE", 0) != 0 && grid.x > 8) {
    auto gcd = [](unsigned x, unsigned y) { while (y) { const unsigned t = x % y; x = y; y = t; } return x; };
    unsigned st = (unsigned)(0.6180339887 * grid.x) | 1u;
    while (gcd(st, grid.x) != 1) st += 2;
    a.block_stride = (int)st;
  }
  unsigned long long* wave_log = nullptr;  // laboratory, development: per-wave time and step counts
  if constexpr (kLabBuild) {
    if (a_in.fast && knobs.wave_log) {
      wave_log = wave_log_alloc(s, grid.x);
      if (!wave_log) return hipErrorOutOfMemory;
      a.wave_log = wave_log;
    }
  }
  rt = choose_tile_route(sizeof(T) == 8, a_in.fast != 0, knobs);
  hipError_t e = hipErrorInvalidValue;
  if (rt.rows >= 0) {
    e = launch_walk_tile_rows<T>(k, a, rt);
  } else if (rt.rec_mode >= 0) {
    e = launch_walk_tile_fast<T>(k, a, rt);
  } else if constexpr (kLabBuild && sizeof(T) == 4) {  // "fast-bfs": f32 (in index order: the chunk ordering is off whenever it is asked for)
    e = launch_walk_tile_fast_bfs(k, a);
  }
  if constexpr (kLabBuild) {
    if (wave_log) wave_log_dump(s, wave_log, grid.x);
  }
  return e;
}

template <class T>
hipError_t launch_tree_walk_tile(hipStream_t s, const WalkArgs<T>& a, char* scratch, const WalkSplitLayout& L, const uint32_t* tgt_ids,
                                 uint32_t* hist, int estimate, int shift, TileRoute* route) {
  int64_t waves = 0;
  hipError_t e = launch_tree_walk_tile_prep<T>(s, a, scratch, L, tgt_ids, hist, estimate, shift, &waves, nullptr);
  if (e != hipSuccess) return e;
  return launch_tree_walk_tile_main<T>(s, a, scratch, L, tgt_ids, hist, waves, route);
}

template hipError_t launch_tree_walk_tile<float>(hipStream_t, const WalkArgs<float>&, char*, const WalkSplitLayout&, const uint32_t*, uint32_t*, int, int, TileRoute*);
template hipError_t launch_tree_walk_tile<double>(hipStream_t, const WalkArgs<double>&, char*, const WalkSplitLayout&, const uint32_t*, uint32_t*, int, int, TileRoute*);
template hipError_t launch_tree_walk_tile_main<float>(hipStream_t, const WalkArgs<float>&, char*, const WalkSplitLayout&, const uint32_t*, uint32_t*, int64_t, TileRoute*);
template hipError_t launch_tree_walk_tile_main<double>(hipStream_t, const WalkArgs<double>&, char*, const WalkSplitLayout&, const uint32_t*, uint32_t*, int64_t, TileRoute*);

}  // namespace nbody
