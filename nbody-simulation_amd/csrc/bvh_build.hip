// Device-side build of the linearised BVH (gfx950, f32) — bit-identical to the host builder (tree_build.hpp) and to
// BVHTree::from + calculate_gravity of /root/reference src/bvh_tree.rs:40-158.
//
// What has to be reproduced, per node (bvh_tree.rs:56-96): ONE sequential fold over the slice (min from f32::MAX, max
// from 0.0, sum in slice order), mean = sum / len, the "better balanced axis" rule on #{x > mean.x} / #{y > mean.y},
// and the two-pointer partition of crate `partition` 0.1.2 (predicate-true side first).  The order of the particles
// inside each side feeds the next level's sum, so the permutation has to be exact, not just the split.
//
//   * min / max / counts are order-independent: plain reductions.
//   * the sum is a rounding chain: exact_sum.h (here its float instance) scans it (addend = map parity -> increment
//     inside one binade; a real f32 add whenever the chain leaves its binade).
//   * the two-pointer partition swaps the k-th misplaced element from the left with the k-th misplaced element from
//     the right (the pointers only ever stop at misplaced elements): two rank lists from one prefix count, then
//     independent swaps.
//
// Two phases.  Nodes longer than kSub points are processed breadth-first, a level at a time, with the node's points
// spread over many work-groups: bvh_big_fold (the chain: one 512-thread group per node and coordinate, the only serial part),
// bvh_big_count (per-chunk counts; the last chunk to finish picks the axis, the split and creates the children),
// bvh_big_ranks (ranks from the predicate bits bvh_big_count left; the two halves of a pair meet in a 64-bit slot and whoever
// arrives second swaps: round 3, one launch per level fewer).  Every node of at most kSub points is the root of a subtree that ONE
// work-group builds completely out of LDS (bvh_subtrees): long nodes by the whole group, short ones a wave each.
//
// Nodes get breadth-first ids while they are made.  The upward pass (:133-158; leaves: unweighted mean in slice order,
// u32 wrapping mass, :98-131) also counts the nodes of every subtree; the pre-order index the walk needs follows top-down
// (node, left subtree, right subtree) for the nodes above the subtrees, and by a walk up to the nearest numbered ancestor
// for the others; `skip` = index + subtree size.
//
// Anything this cannot express (NaN positions — pathfinder's minps/maxps are order-dependent there —, a node deeper than
// the 56-bit path, more nodes than the buffers hold) raises a flag and the caller uses the host builder instead.
//
// Where the code is: bvh_device.h (what the units share on the device), bvh_fold.hip (the chain), bvh_partition.hip (count,
// ranks, swaps), bvh_subtrees.hip, bvh_finish.hip (upward pass, numbering, final arrays); bvh_units.h declares their launchers.
// This file: the scratch layout, bvh_init, and the three host entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_device.h"
#include "bvh_units.h"

namespace nbody {

namespace {

// ---- init --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bvh_init(BvhPtrs a, const float2* __restrict__ pos, int n, unsigned long long* __restrict__ stamp_begin,
                                                unsigned long long* __restrict__ stamp_prev_end) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0 && (stamp_begin || stamp_prev_end)) {  // phase clock (tree_driver.hip, stamp_*): this step begins where the one before ends
    const unsigned long long now = (unsigned long long)wall_clock64();
    if (stamp_begin) *stamp_begin = now;
    if (stamp_prev_end) *stamp_prev_end = now;
  }
  if (i < n) {
    const float2 p = pos[i];
    a.P[i] = p;
    a.ID[i] = (uint32_t)i;
    a.pair[i] = 0ull;  // (the pair slots clean themselves; a build that was abandoned half-way may have left some)
    if (p.x != p.x || p.y != p.y) a.flags[kBvhFallback] = 1;
  }
  for (int j = i + 1; j < a.cap; j += gridDim.x * 256) a.ndepth[j] = -1;  // not a node (yet): ids are handed out in ranges
  if (n > kSub && i < (n + kChunk - 1) / kChunk) {  // the root's chunks
    a.ch_rec[i] = make_int4(0, i, 0, n);
  }
  if (i == 0) {  // the top call is unconditional: the root is a Root whatever its length (main.rs:400)
    a.nbegin[0] = 0;
    a.nlen[0] = n;
    a.nparent[0] = -1;
    a.nchild[0] = -1;
    a.ndepth[0] = 0;
    a.nleaf[0] = 0;
    a.npre[0] = 0;  // the root comes first
    a.ndone[0] = 0;
    a.nbad[0] = 0;
    a.flags[kBvhNodeCount] = 1;
    a.flags[kBvhTopCount] = 1;
    a.topq[0] = 0;
    if (n > kSub) {
      a.bigcount[0] = 1;
      a.bigq[0] = 0;
      a.chunkcount[0] = (n + kChunk - 1) / kChunk;
      a.nchunk0[0] = 0;
    } else {
      a.flags[kBvhSubCount] = 1;
      a.subq[0] = 0;
    }
  }
}

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

BvhBuildLayout bvh_build_layout(int64_t n, int leaf_size) {
  BvhBuildLayout L{};
  const size_t N = (size_t)(n > 0 ? n : 1);
  // leaves end up between half full and full: ~2.7 N / leaf_size nodes.  More than this -> host builder
  const size_t lf = (size_t)(leaf_size > 0 ? leaf_size : 1);
  const size_t C = (4 * N / lf < 2 * N ? 4 * N / lf : 2 * N) + 4096;
  const size_t CB = N / (size_t)(kSub + 1) + 2;      // long nodes of one level
  const size_t CC = N / (size_t)kChunk + CB + 2;     // their chunks
  L.node_cap = (int)C;
  L.big_cap = (int)CB;
  L.chunk_cap = (int)CC;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
  L.flags = take(sizeof(int) * kBvhFlagWords);
  L.bigcount = take(sizeof(int) * kBvhLevels);
  L.chunkcount = take(sizeof(int) * kBvhLevels);
  L.zero_end = off;
  L.bigq = take(4 * 2 * CB);
  L.subq = take(4 * C);
  L.topq = take(4 * C);
  L.ch_rec = take(16 * 2 * CC);
  L.ch_sum = take(16 * CC);
  L.ch_box = take(16 * CC);
  L.ch_run = take(4 * 48 * CC);  // 2 * kRunRec ints per chunk (bvh_fold.hip)
  L.ch_cx = take(4 * CC);
  L.ch_cy = take(4 * CC);
  L.ch_before = take(4 * CC);
  L.pts = take(sizeof(float2) * N);
  L.ids = take(4 * N);
  L.lidx = take(4 * N);
  L.ridx = take(4 * N);
  L.pred = take(N);
  L.pair = take(8 * N);
  L.nbegin = take(4 * C);
  L.nlen = take(4 * C);
  L.nparent = take(4 * C);
  L.nchild = take(4 * C);
  L.ndepth = take(4 * C);
  L.nleaf = take(4 * C);
  L.nsize = take(4 * C);
  L.npre = take(4 * C);
  L.nbox = take(16 * C);
  L.ncog = take(8 * C);
  L.nmass = take(4 * C);
  L.narrive = take(4 * C);
  L.nmean = take(8 * C);
  L.nsplit = take(4 * C);
  L.nchunk0 = take(4 * C);
  L.ndone = take(4 * C);
  L.nbad = take(4 * C);
  L.total = off;
  return L;
}

int bvh_build_first_levels(int64_t n) {
  int lv = 0;
  for (int64_t k = kSub; k < n; k *= 2) ++lv;  // a balanced tree's long levels
  return lv;
}

hipError_t bvh_build_begin(hipStream_t s, const void* pos, int n, char* scratch, const BvhBuildLayout& L, bool flags_clean,
                           unsigned long long* stamp_begin, unsigned long long* stamp_prev_end) {
  hipError_t e = flags_clean ? hipSuccess : hipMemsetAsync(scratch + L.flags, 0, L.zero_end - L.flags, s);  // flags + level counters
  if (e != hipSuccess) return e;
  BvhPtrs a = make_ptrs(scratch, L);
  bvh_init<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(a, (const float2*)pos, n, stamp_begin, stamp_prev_end);
  return hipGetLastError();
}

hipError_t bvh_build_levels(hipStream_t s, int n, int leaf_size, int level_begin, int level_end, char* scratch,
                            const BvhBuildLayout& L) {
  for (int level = level_begin; level < level_end && level < kBvhLevels - 1; ++level) {
    const int64_t width = level < 30 ? (int64_t)1 << level : (int64_t)1 << 30;  // a level never has more nodes than this
    int64_t gb = L.big_cap < width ? L.big_cap : width;
    int64_t gc = L.chunk_cap;
    if (gc > 1024) gc = 1024;
    // could a node of this level be longer than kRunLen?  (A performance choice only: a chain without prepared runs is
    // scanned.  Three quarters of kRunLen as the level's average: the level whose nodes average 9 462 of the reference scene's
    // points spent two launches preparing runs nobody used.)
    const int use_runs = (n >> level) > kRunLen * 3 / 4 ? 1 : 0;
    if (use_runs) {
      launch_bvh_chunk_sums(s, scratch, L, gc, level);
      launch_bvh_chunk_runs(s, scratch, L, gc, level);
    }
    launch_bvh_big_fold(s, scratch, L, gb, level, use_runs);
    launch_bvh_big_count(s, scratch, L, gc, level, leaf_size);
    if (n <= kFusedPartitionMax) {
      launch_bvh_big_ranks(s, scratch, L, gc, level);
    } else {
      launch_bvh_big_ranks_lists(s, scratch, L, gc, level);
      launch_bvh_big_swap(s, scratch, L, gc, level);
    }
  }
  return hipGetLastError();
}

hipError_t bvh_build_finish(hipStream_t s, const uint32_t* weight, int n, int leaf_size, int sub_start, char* scratch,
                            const BvhBuildLayout& L,
                            uint32_t* order_out, void* geom0, void* geom1, void* link, int* depth_out, uint32_t* mass_out,
                            float2* size_out, const GatherArgs<float>* gather) {
  const int C = L.node_cap;
  int64_t gs = (int64_t)n / 64 + 1;  // subtree roots
  if (gs > 2048) gs = 2048;
  launch_bvh_subtrees(s, scratch, L, gs, weight, leaf_size, sub_start);
  launch_bvh_top_upward(s, scratch, L, weight);
  const dim3 gm((unsigned)((C + 255) / 256));
  if (gather && gather->n > 0) {  // the rows into tree order in the same launch (perm: where the build left it, bvh_build_order)
    launch_bvh_emit_gather(s, scratch, L, gm, geom0, geom1, link, depth_out, mass_out, size_out, *gather);
  } else {
    launch_bvh_emit(s, scratch, L, gm, geom0, geom1, link, depth_out, mass_out, size_out);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!order_out) return hipSuccess;
  return hipMemcpyAsync(order_out, bvh_build_order(scratch, L), sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, s);
}
const uint32_t* bvh_build_order(const char* scratch, const BvhBuildLayout& L) { return (const uint32_t*)(scratch + L.ids); }

}  // namespace nbody
