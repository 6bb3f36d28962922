// What the units of the big-leaf BVH walk offer one another on the host: one launcher per kernel family, each taking the
// TileRoute that walk_launch.hip chose (walk_route.h), and the laboratory's side duties.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tree_kernels.h"
#include "walk_split.h"

namespace nbody {

// what every one-pass walk kernel is launched with, besides its WalkArgs
struct TileLaunch {
  hipStream_t s;
  dim3 grid;  // work-groups of four waves
  const uint32_t* off;
  int* info;
  const uint32_t* tgt_ids;
  uint32_t* hist;
  unsigned long long* total_out;
};

// A route that names an instantiation this build does not hold (the product ships rows 8 with scalar node records, the f32
// register walk with record mode 3, and the f64 rows arm for FAST) is hipErrorInvalidValue.
template <class T> hipError_t launch_walk_tile_rows(const TileLaunch& k, const WalkArgs<T>& a, const TileRoute& rt);  // walk_tile.hip: "exact", "fast-rows"
template <class T> hipError_t launch_walk_tile_fast(const TileLaunch& k, const WalkArgs<T>& a, const TileRoute& rt);  // walk_tile_fast.hip: "fast-registers", "fast-registers-log"

// walk_prepare.hip: off = the exclusive scan of cnt, info[1] and info[2] set if the 32-bit sums wrapped
hipError_t launch_walk_count_scan(hipStream_t s, char* scratch, const WalkSplitLayout& L, int64_t n_tgt);

// walk_lab.hip: defined in the laboratory build only
hipError_t launch_walk_tile_fast_bfs(const TileLaunch& k, const WalkArgs<float>& a);  // "fast-bfs"
struct ChunkOrder {
  const int* order;  // WalkArgs::group_order
  int chunk;         // WalkArgs::order_chunk
  unsigned groups;   // the grid: whole chunks
};
ChunkOrder launch_walk_order_chunks(hipStream_t s, const uint32_t* off, int n_tgt, const int* info, unsigned n_groups, int* order, int mode);
unsigned long long* wave_log_alloc(hipStream_t s, unsigned n_groups);  // WalkArgs::wave_log, zeroed; null: out of memory
void wave_log_dump(hipStream_t s, unsigned long long* wave_log, unsigned n_groups);  // waits for the stream, writes the file, frees

}  // namespace nbody
