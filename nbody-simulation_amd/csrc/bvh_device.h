// What the units of the device-side BVH build (f32) share on the device (bvh_build.hip, bvh_fold.hip, bvh_partition.hip,
// bvh_subtrees.hip, bvh_finish.hip): the build-time constants, the scratch pointers, and the helpers that two or more of the
// units use.  A helper that one unit alone uses lives in that unit.  The design is described at the top of bvh_build.hip.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_build.h"
#include "tree_kernels.h"
#include "exact_sum.h"

namespace nbody {

namespace {

using Chain = xsum::Chain<float>;  // this build is the f32 one
using Step = xsum::Step<float>;
using Run = xsum::Run<float>;

// The three NB_* defaults live here so that a -D on the command line reaches every unit.  No unit uses every constant.
[[maybe_unused]] constexpr int kEPT = 4;          // consecutive points per thread in the rank-list passes
[[maybe_unused]] constexpr int kSeqRun = 16;      // real adds after every stop of the scan
#ifndef NB_CHAIN_START
#define NB_CHAIN_START 512
#endif
[[maybe_unused]] constexpr int kChainStart = NB_CHAIN_START; // real adds at the start of a long node's chain (the sum doubles too often there)
#ifndef NB_KSUB
#define NB_KSUB 2048
#endif
[[maybe_unused]] constexpr int kSub = NB_KSUB;       // nodes up to this long are built, subtree and all, by one work-group in LDS
[[maybe_unused]] constexpr int kSubWaves = 8;     // waves of a subtree work-group
[[maybe_unused]] constexpr int kChunk = 2048;     // points per work-group in the multi-group passes over a long node
#ifndef NB_RUN_LEN
#define NB_RUN_LEN 16384
#endif
[[maybe_unused]] constexpr int kFusedPartitionMax = 400000;  // points up to which a level's rank pass also swaps (bvh_big_ranks); beyond: lists + bvh_big_swap
[[maybe_unused]] constexpr int kRunLen = NB_RUN_LEN;   // nodes longer than this have their chain prepared chunk by chunk (bvh_chunk_runs)
[[maybe_unused]] constexpr float kMaxF = 3.402823466e+38f;

struct BvhPtrs {
  int* flags;
  int* bigcount;    // [level]: long nodes queued for the level
  int* chunkcount;  // [level]
  int* bigq;        // [level & 1][cap_big]
  int* subq;        // subtree roots
  int* topq;        // nodes made by the long-node levels (the ones above the subtrees)
  int4* ch_rec;     // [level & 1][cap_chunk] chunk -> node, index inside the node, the node's begin and length (one load
                    // tells a chunk's kernel where its points are: the node's other fields and the points travel together)
  double2* ch_sum;  // exact-ish (f64) sums of the chunk's coordinates: only used to PREDICT binades
  float4* ch_box;   // min.x min.y max.x max.y of the chunk
  int* ch_run;      // [chunk][2 coordinates][kRunRec]: see bvh_chunk_runs
  int* ch_cx;
  int* ch_cy;
  int* ch_before;   // predicate-true points of the node before the chunk
  float2* P;
  uint32_t* ID;
  int* lidx;
  int* ridx;
  uint8_t* pred;             // long nodes: bit 0 = x > mean.x, bit 1 = y > mean.y of every point (bvh_big_count), read by bvh_big_ranks
  unsigned long long* pair;  // long nodes: one slot per pair of misplaced points (low word: the left one's index + 1, high word: the right one's)
  int* nbegin;
  int* nlen;
  int* nparent;
  int* nchild;
  int* ndepth;
  int* nleaf;
  int* nsize;  // nodes in the subtree (the node itself included)
  int* npre;   // pre-order index, -1 while unknown
  float4* nbox;  // min.x, min.y, max.x, max.y
  float2* ncog;
  uint32_t* nmass;
  int* narrive;
  float2* nmean;
  int* nsplit;   // long nodes: m | axis << 31
  int* nchunk0;
  int* ndone;
  int* nbad;
  int cap, cap_big, cap_chunk;
};

BvhPtrs make_ptrs(char* s, const BvhBuildLayout& L) {
  BvhPtrs a;
  a.flags = (int*)(s + L.flags);
  a.bigcount = (int*)(s + L.bigcount);
  a.chunkcount = (int*)(s + L.chunkcount);
  a.bigq = (int*)(s + L.bigq);
  a.subq = (int*)(s + L.subq);
  a.topq = (int*)(s + L.topq);
  a.ch_rec = (int4*)(s + L.ch_rec);
  a.ch_sum = (double2*)(s + L.ch_sum);
  a.ch_box = (float4*)(s + L.ch_box);
  a.ch_run = (int*)(s + L.ch_run);
  a.ch_cx = (int*)(s + L.ch_cx);
  a.ch_cy = (int*)(s + L.ch_cy);
  a.ch_before = (int*)(s + L.ch_before);
  a.P = (float2*)(s + L.pts);
  a.ID = (uint32_t*)(s + L.ids);
  a.lidx = (int*)(s + L.lidx);
  a.ridx = (int*)(s + L.ridx);
  a.pred = (uint8_t*)(s + L.pred);
  a.pair = (unsigned long long*)(s + L.pair);
  a.nbegin = (int*)(s + L.nbegin);
  a.nlen = (int*)(s + L.nlen);
  a.nparent = (int*)(s + L.nparent);
  a.nchild = (int*)(s + L.nchild);
  a.ndepth = (int*)(s + L.ndepth);
  a.nleaf = (int*)(s + L.nleaf);
  a.nsize = (int*)(s + L.nsize);
  a.npre = (int*)(s + L.npre);
  a.nbox = (float4*)(s + L.nbox);
  a.ncog = (float2*)(s + L.ncog);
  a.nmass = (uint32_t*)(s + L.nmass);
  a.narrive = (int*)(s + L.narrive);
  a.nmean = (float2*)(s + L.nmean);
  a.nsplit = (int*)(s + L.nsplit);
  a.nchunk0 = (int*)(s + L.nchunk0);
  a.ndone = (int*)(s + L.ndone);
  a.nbad = (int*)(s + L.nbad);
  a.cap = L.node_cap;
  a.cap_big = L.big_cap;
  a.cap_chunk = L.chunk_cap;
  return a;
}

// pathfinder_simd min/max on SSE: `a < b ? a : b` (second operand when unordered); NaNs never get here
__device__ __forceinline__ float sse_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float sse_max(float a, float b) { return a > b ? a : b; }

// ---- the chain, one add after the other -----------------------------------------------------------------------------
struct Box {
  float mnx = kMaxF, mny = kMaxF, mxx = 0.f, mxy = 0.f;  // the fold's start values, bvh_tree.rs:42, :59
  __device__ __forceinline__ void add(float2 q) {
    mnx = sse_min(mnx, q.x); mny = sse_min(mny, q.y);
    mxx = sse_max(mxx, q.x); mxy = sse_max(mxy, q.y);
  }
  __device__ __forceinline__ void reduce_wave() {
    for (int d = 32; d >= 1; d >>= 1) {
      mnx = sse_min(mnx, __shfl_xor(mnx, d, 64)); mny = sse_min(mny, __shfl_xor(mny, d, 64));
      mxx = sse_max(mxx, __shfl_xor(mxx, d, 64)); mxy = sse_max(mxy, __shfl_xor(mxy, d, 64));
    }
  }
};
// s + X[0] + X[STRIDE] + ... (count addends, in order) from LDS, the same address in every lane (a broadcast read); count
// uniform.  The adds depend on one another, the reads do not: the next 16 words are on their way while these 16 are added,
// else every batch waits out the LDS latency (13+ clocks per addend instead of the 4-5 of a dependent add).  Two register
// sets taken in turn; the sched_group_barriers keep the scheduler from sinking the reads below the adds they overlap.
#define NB_CHAIN_LOAD(dst, from) _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) dst[j_] = X[STRIDE * ((from) + j_)];
#define NB_CHAIN_ADD(src) _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) s = s + src[j_]; \
  __builtin_amdgcn_sched_group_barrier(0x100, 16, 0); __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
template <int STRIDE>
__device__ __forceinline__ float chain_lds(const float* X, int count, float s) {
  count = __builtin_amdgcn_readfirstlane(count);
  int k = 0;
  if (count >= 16) {
    float va[16], vb[16];
    NB_CHAIN_LOAD(va, 0)
    for (; k + 48 <= count; k += 32) {  // va holds [k, k + 16) here
      NB_CHAIN_LOAD(vb, k + 16)
      NB_CHAIN_ADD(va)
      NB_CHAIN_LOAD(va, k + 32)
      NB_CHAIN_ADD(vb)
    }
    if (k + 32 <= count) {
      NB_CHAIN_LOAD(vb, k + 16)
      NB_CHAIN_ADD(va)
      NB_CHAIN_ADD(vb)
      k += 32;
    } else {
      NB_CHAIN_ADD(va)
      k += 16;
    }
  }
  for (; k < count; ++k) s = s + X[STRIDE * k];
  return s;
}
#undef NB_CHAIN_LOAD
#undef NB_CHAIN_ADD

// ---- NW waves working on one node --------------------------------------------------------------------------------
// NW == 1 needs no barrier and no LDS (a wave runs in lock-step); NW > 1 is a whole work-group.
template <int NW> __device__ __forceinline__ unsigned group_sum(unsigned v, unsigned* slot, int tid) {
  for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
  if constexpr (NW == 1) {
    return v;
  } else {
    if ((tid & 63) == 0) slot[tid >> 6] = v;
    __syncthreads();
    unsigned t = 0;
    for (int w = 0; w < NW; ++w) t += slot[w];
    __syncthreads();
    return t;
  }
}

// :70-73 — which axis splits closer to the middle; returns the split point m (predicate-true side comes first)
__device__ __forceinline__ int choose_axis(int len, int cxs, int cys, bool& on_x) {
  const int half = len / 2;
  const int hori = half > cxs ? half - cxs : cxs - half;
  const int vert = half > cys ? half - cys : cys - half;
  on_x = vert > hori;
  return on_x ? cxs : cys;
}

// Children of `node` ([b, b+m) and [b+m, b+len)) with the ids first, first + 1: records and keys.  One thread.
// leaf[] says which children need no further splitting.
// depth_max: where the tree's depth is collected; null: the global flag, one atomic per node (the subtree kernel collects per
// work-group in LDS and reports once: thousands of atomics on one address are the slowest thing a build can do).
__device__ __forceinline__ void make_children(const BvhPtrs& a, int node, int first, int b, int len, int m, int leaf_size,
                                              bool leaf[2], int* depth_max = nullptr, int depth = -1) {
  const int d = depth >= 0 ? depth : a.ndepth[node];  // (a caller that knows the node's depth saves the trip to memory)
  a.nchild[node] = first;
  for (int side = 0; side < 2; ++side) {
    const int id = first + side;
    const int cl = side ? len - m : m;
    a.nbegin[id] = side ? b + m : b;
    a.nlen[id] = cl;
    a.nparent[id] = node;
    a.nchild[id] = -1;
    a.ndepth[id] = d + 1;
    bool lf = !(cl > leaf_size);  // :78-88
    if (!lf && d + 1 >= kBvhKeyDepth) { a.flags[kBvhFallback] = 1; lf = true; }
    leaf[side] = lf;
    a.nleaf[id] = lf ? 1 : 0;
    a.npre[id] = -1;
    a.ndone[id] = 0;
    a.nbad[id] = 0;
  }
  atomicMax(depth_max ? depth_max : &a.flags[kBvhMaxDepth], d + 1);
}
// two fresh node ids, or -1 with the fallback flag up when the buffers are full
__device__ __forceinline__ int alloc_nodes(const BvhPtrs& a, int count) {
  const int first = atomicAdd(&a.flags[kBvhNodeCount], count);
  if (first + count > a.cap) {
    a.flags[kBvhFallback] = 1;
    return -1;
  }
  return first;
}

// Centre and mass of an internal node from its two children (bvh_tree.rs:133-158)
__device__ __forceinline__ void combine_children(const BvhPtrs& a, int node) {
  const int c0 = a.nchild[node];
  if (c0 < 0) {  // children not made (yet: a blind pass on an unfinished tree; or buffers full, the fallback flag is up)
    a.nsize[node] = 1;
    return;
  }
  const float2 g0 = a.ncog[c0], g1 = a.ncog[c0 + 1];
  const uint32_t m0 = a.nmass[c0], m1 = a.nmass[c0 + 1];
  const uint32_t ms = m0 + m1;                                      // :148
  const float bx = (g0.x * (float)m0) + (g1.x * (float)m1);         // :150-153
  const float by = (g0.y * (float)m0) + (g1.y * (float)m1);
  a.ncog[node] = make_float2(bx / (float)ms, by / (float)ms);       // :154
  a.nmass[node] = ms;
  a.nsize[node] = 1 + a.nsize[c0] + a.nsize[c0 + 1];
}

}  // namespace

}  // namespace nbody
