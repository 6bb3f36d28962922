// The subtrees of the device-side BVH build (f32, design: bvh_build.hip): every node of at most kSub points is the root of a
// subtree that one work-group builds completely out of LDS, leaves and upward pass included.  All of NB_BVH_TIMING is here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_device.h"
#include "bvh_units.h"

namespace nbody {

namespace {

// both coordinates of P[0 .. count) at once (two independent chains share the reads)
__device__ __forceinline__ void chain_lds_xy(const float2* P, int count, float& sx, float& sy) {
  count = __builtin_amdgcn_readfirstlane(count);
  int k = 0;
#define NB_CHAIN_LOAD(dst, from) _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) dst[j_] = P[(from) + j_];
#define NB_CHAIN_ADD(src) _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) { sx = sx + src[j_].x; sy = sy + src[j_].y; } \
  __builtin_amdgcn_sched_group_barrier(0x100, 8, 0); __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
  if (count >= 8) {
    float2 va[8], vb[8];
    NB_CHAIN_LOAD(va, 0)
    for (; k + 24 <= count; k += 16) {  // va holds [k, k + 8) here
      NB_CHAIN_LOAD(vb, k + 8)
      NB_CHAIN_ADD(va)
      NB_CHAIN_LOAD(va, k + 16)
      NB_CHAIN_ADD(vb)
    }
    if (k + 16 <= count) {
      NB_CHAIN_LOAD(vb, k + 8)
      NB_CHAIN_ADD(va)
      NB_CHAIN_ADD(vb)
      k += 16;
    } else {
      NB_CHAIN_ADD(va)
      k += 8;
    }
  }
#undef NB_CHAIN_LOAD
#undef NB_CHAIN_ADD
  for (; k < count; ++k) { sx = sx + P[k].x; sy = sy + P[k].y; }
}

template <int NW> __device__ __forceinline__ void group_sync() {
  if constexpr (NW > 1) {
    __syncthreads();
  } else {  // LDS written by one lane, read by another lane of the same wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// `count` fresh node ids or -1, without a verdict on the build (the caller has a smaller request to fall back on)
__device__ __forceinline__ int try_alloc_nodes(const BvhPtrs& a, int count) {
  const int first = atomicAdd(&a.flags[kBvhNodeCount], count);
  if (first + count > a.cap) {
    atomicSub(&a.flags[kBvhNodeCount], count);
    return -1;
  }
  return first;
}

// ---- subtrees of at most kSub points, entirely in LDS -----------------------------------------------------------------
struct SubLds {
  float2 P[kSub];
  uint16_t I[kSub];  // which of the subtree's points (as loaded) sits here now
  uint32_t W[kSub];  // weights of the points as loaded
  uint16_t L[kSub], R[kSub];
  uint16_t lb[2][kSub / 2], ll[2][kSub / 2];  // node lists of two consecutive levels: begin, length (subtree-relative)
  int lg[2][kSub / 2];                        // ... and breadth-first id
  int lcount[2];
  // ids of the children made at this level: pair e (children of the level's e-th node) takes idbase + 2 e while 2 e < idsplit
  // (what was left of the range the work-group held) and idbase2 + 2 e - idsplit after that (the head of a new range)
  int idbase, idsplit, idbase2;
  int depth_max;  // deepest node made by this work-group
  int id_next, id_end;  // ids this work-group holds (one atomic on the global counter per range, not per level)
  int loff[kBvhKeyDepth + 2];  // where each level of the subtree starts in its list of internal nodes
  // nodes_by_groups: per wave partial results, per node sums
  float4 gbox[kSubWaves];
  float2 gsum[kSubWaves];
  unsigned gcx[kSubWaves], gcy[kSubWaves], gtot[kSubWaves], gbad[kSubWaves];
};

struct LevelIds {  // (a copy in registers: the three words are read once per level, side by side)
  int base, split, base2;
  __device__ __forceinline__ int pair_first(int e) const { return 2 * e < split ? base + 2 * e : base2 + 2 * e - split; }
};

// One node whose points are s.P[lb, lb+len): fold, axis, partition, children — by ONE wave.  Up to kSub points the
// chain is simply added in order (a scan would restart at every doubling of the sum and lose).
__device__ __forceinline__ void node_in_lds(const BvhPtrs& a, SubLds& s, int gbegin, int lb, int len, int gid, int first, int lane,
                                            int nxt, int leaf_size, int depth) {
  constexpr int TILE = 64 * kEPT;
  float2* P = s.P + lb;
  uint16_t* I = s.I + lb;
  uint16_t* L = s.L + lb;
  uint16_t* R = s.R + lb;
  // the chain: every lane reads the same LDS word (a broadcast) and adds it — 8 clocks per add, measured against 14 for
  // the DPP broadcast and 10 for v_readlane (tools/chain_microbench.hip)
  float sx = 0.f, sy = 0.f;
  chain_lds_xy(P, len, sx, sy);
  const float hx = sx / (float)len, hy = sy / (float)len;  // :67
  Box box;
  unsigned cx = 0u, cy = 0u;
  for (int i = lane; i < len; i += 64) {
    const float2 q = P[i];
    box.add(q);
    cx += q.x > hx;
    cy += q.y > hy;
  }
  box.reduce_wave();
  cx = group_sum<1>(cx, nullptr, lane);
  cy = group_sum<1>(cy, nullptr, lane);
  bool on_x;
  const int m = choose_axis(len, (int)cx, (int)cy, on_x);
  unsigned carry = 0u, nbad = 0u;
  for (int p0 = 0; p0 < len; p0 += TILE) {
    const int base = p0 + lane * kEPT;
    bool pr[kEPT];
    unsigned mine = 0u;
#pragma unroll
    for (int j = 0; j < kEPT; ++j) {
      pr[j] = false;
      if (base + j < len) {
        const float2 q = P[base + j];
        pr[j] = on_x ? q.x > hx : q.y > hy;
        mine += pr[j];
      }
    }
    unsigned inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += o;
    }
    const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);
    unsigned t = carry + inc - mine;
#pragma unroll
    for (int j = 0; j < kEPT; ++j) {
      const int i = base + j;
      if (i < len) {
        if (i < m && !pr[j]) { L[i - (int)t] = (uint16_t)i; ++nbad; }
        else if (i >= m && pr[j]) R[m - (int)t - 1] = (uint16_t)i;
        t += pr[j];
      }
    }
    carry += total;
  }
  nbad = group_sum<1>(nbad, nullptr, lane);
  group_sync<1>();
  for (int k = lane; k < (int)nbad; k += 64) {
    const int l = L[k], r = R[k];
    const float2 pl = P[l], pr = P[r];
    P[l] = pr; P[r] = pl;
    const uint16_t il = I[l], ir = I[r];
    I[l] = ir; I[r] = il;
  }
  if (lane == 0) {
    a.nbox[gid] = make_float4(box.mnx, box.mny, box.mxx, box.mxy);
    bool leaf[2];
    make_children(a, gid, first, gbegin + lb, len, m, leaf_size, leaf, &s.depth_max, depth);
    for (int side = 0; side < 2; ++side) {
      if (leaf[side]) continue;
      const int slot = atomicAdd(&s.lcount[nxt], 1);
      s.lb[nxt][slot] = (uint16_t)(side ? lb + m : lb);
      s.ll[nxt][slot] = (uint16_t)(side ? len - m : m);
      s.lg[nxt][slot] = first + side;
    }
  }
  group_sync<1>();
}

// The first levels of a subtree have fewer nodes than the work-group has waves: G waves share a node (nc * G <= kSubWaves).
// What node_in_lds does, spread out: the two chains (one add after the other) get a wave each; box, counts, rank lists and
// swaps are split G ways.  Every wave runs the same number of barriers
// (the longest node of the level sets the number of rank-list rounds).
template <int G>
__device__ __forceinline__ void nodes_by_groups(const BvhPtrs& a, SubLds& s, int gbegin, int cur, int nc, LevelIds ids, int tid,
                                                int leaf_size, int depth) {
  static_assert(G >= 2 && kSubWaves % G == 0, "at least one wave beside the chain's");
  constexpr int TILE = 64 * kEPT;
  const int lane = tid & 63, wave = tid >> 6;
  const int grp = wave / G, gw = wave % G, w0 = grp * G;
  const bool act = grp < nc;
  const int lb = act ? s.lb[cur][grp] : 0, len = act ? s.ll[cur][grp] : 0, gid = act ? s.lg[cur][grp] : 0;
  int maxlen = 0;
  for (int e = 0; e < nc; ++e) maxlen = maxlen > (int)s.ll[cur][e] ? maxlen : (int)s.ll[cur][e];
  float2* P = s.P + lb;
  uint16_t* I = s.I + lb;
  uint16_t* L = s.L + lb;
  uint16_t* R = s.R + lb;
  // the two chains, a wave each (one dependent add per point instead of two)
  if (gw < 2) {
    const float sc = chain_lds<2>(reinterpret_cast<const float*>(P) + gw, len, 0.f);
    if (lane == 0) (gw ? s.gsum[grp].y : s.gsum[grp].x) = sc;
  }
  __syncthreads();
  const float2 sum = s.gsum[grp];
  const float hx = sum.x / (float)len, hy = sum.y / (float)len;  // :67
  Box box;
  unsigned cx = 0u, cy = 0u;
  for (int i = gw * 64 + lane; i < len; i += G * 64) {
    const float2 q = P[i];
    box.add(q);
    cx += q.x > hx;
    cy += q.y > hy;
  }
  box.reduce_wave();
  cx = group_sum<1>(cx, nullptr, lane);
  cy = group_sum<1>(cy, nullptr, lane);
  if (lane == 0) {
    s.gbox[wave] = make_float4(box.mnx, box.mny, box.mxx, box.mxy);
    s.gcx[wave] = cx;
    s.gcy[wave] = cy;
  }
  __syncthreads();
  cx = 0u; cy = 0u;
  box = Box();
  for (int w = 0; w < G; ++w) {
    const float4 bx = s.gbox[w0 + w];
    box.mnx = sse_min(box.mnx, bx.x); box.mny = sse_min(box.mny, bx.y);
    box.mxx = sse_max(box.mxx, bx.z); box.mxy = sse_max(box.mxy, bx.w);
    cx += s.gcx[w0 + w];
    cy += s.gcy[w0 + w];
  }
  bool on_x;
  const int m = choose_axis(len, (int)cx, (int)cy, on_x);
  unsigned carry = 0u, nbad = 0u;
  for (int r0 = 0; r0 < maxlen; r0 += G * TILE) {
    const int base = r0 + gw * TILE + lane * kEPT;
    bool pr[kEPT];
    unsigned mine = 0u;
#pragma unroll
    for (int j = 0; j < kEPT; ++j) {
      pr[j] = false;
      if (base + j < len) {
        const float2 q = P[base + j];
        pr[j] = on_x ? q.x > hx : q.y > hy;
        mine += pr[j];
      }
    }
    unsigned inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) s.gtot[wave] = inc;
    __syncthreads();
    unsigned before = carry, total = 0u;
    for (int w = 0; w < G; ++w) {
      const unsigned v = s.gtot[w0 + w];
      if (w < gw) before += v;
      total += v;
    }
    unsigned t = before + inc - mine;
#pragma unroll
    for (int j = 0; j < kEPT; ++j) {
      const int i = base + j;
      if (i < len) {
        if (i < m && !pr[j]) { L[i - (int)t] = (uint16_t)i; ++nbad; }
        else if (i >= m && pr[j]) R[m - (int)t - 1] = (uint16_t)i;
        t += pr[j];
      }
    }
    carry += total;
    __syncthreads();  // gtot is rewritten by the next round; after the last one: the rank lists are complete
  }
  nbad = group_sum<1>(nbad, nullptr, lane);
  if (lane == 0) s.gbad[wave] = nbad;
  __syncthreads();
  nbad = 0u;
  for (int w = 0; w < G; ++w) nbad += s.gbad[w0 + w];
  for (int k = gw * 64 + lane; k < (int)nbad; k += G * 64) {
    const int l = L[k], r = R[k];
    const float2 pl = P[l], pr = P[r];
    P[l] = pr; P[r] = pl;
    const uint16_t il = I[l], ir = I[r];
    I[l] = ir; I[r] = il;
  }
  if (act && gw == 0 && lane == 0) {
    a.nbox[gid] = make_float4(box.mnx, box.mny, box.mxx, box.mxy);
    bool leaf[2];
    const int first = ids.pair_first(grp);
    make_children(a, gid, first, gbegin + lb, len, m, leaf_size, leaf, &s.depth_max, depth);
    const int nxt = cur ^ 1;
    for (int side = 0; side < 2; ++side) {
      if (leaf[side]) continue;
      const int slot = atomicAdd(&s.lcount[nxt], 1);
      s.lb[nxt][slot] = (uint16_t)(side ? lb + m : lb);
      s.ll[nxt][slot] = (uint16_t)(side ? len - m : m);
      s.lg[nxt][slot] = first + side;
    }
  }
}

__global__ __launch_bounds__(kSubWaves * 64) void bvh_subtrees(BvhPtrs a, const uint32_t* __restrict__ weight, int leaf_size,
                                                              int sub_start) {
  __shared__ SubLds s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsub = a.flags[kBvhSubCount];
#ifdef NB_BVH_TIMING
#define NB_STAMP(k) { const long long t_ = wall_clock64(); if (tid == 0) atomicMax(&a.flags[kBvhDebug + k], (int)(t_ - t_prev)); t_prev = t_; }
#else
#define NB_STAMP(k) {}
#endif
  for (int si = sub_start + blockIdx.x; si < nsub; si += gridDim.x) {
#ifdef NB_BVH_TIMING
    long long t_prev = wall_clock64();
#endif
    const int root = a.subq[si];
    const int b = a.nbegin[root], len = a.nlen[root], root_depth = a.ndepth[root];
    int* list = a.lidx + b;  // the subtree's internal nodes, level after level (the global rank lists are free now)
    for (int i = tid; i < len; i += kSubWaves * 64) {
      s.P[i] = a.P[b + i];
      s.I[i] = (uint16_t)i;
      s.W[i] = weight[a.ID[b + i]];
    }
    if (tid == 0) {
      s.depth_max = 0;
      s.id_next = s.id_end = 0;
      s.lb[0][0] = 0;
      s.ll[0][0] = (uint16_t)len;  // kSub = 4096 fits
      s.lg[0][0] = root;
      s.lcount[0] = 1;
      s.lcount[1] = 0;
    }
    __syncthreads();
    NB_STAMP(0)
    int cur = 0, nlev = 0, nint = 0;
    for (;;) {
      const int nc = s.lcount[cur];
      if (nc == 0) break;
      if (nint + nc > len || nlev > kBvhKeyDepth) {  // only degenerate input gets here
        if (tid == 0) a.flags[kBvhFallback] = 1;
        break;
      }
      for (int e = tid; e < nc; e += kSubWaves * 64) list[nint + e] = s.lg[cur][e];
      if (tid == 0) {
        s.loff[nlev] = nint;
        // ids for this level's children out of the work-group's range; a new range when it runs out.  726 work-groups (1 M
        // points) asking the one global counter at every level wait ~60 ns per request ahead of them.
        const int want = 2 * nc;
        const int have = s.id_end - s.id_next;  // (even, like every request: the two children of a node are neighbours)
        s.idbase = s.id_next;
        if (have >= want) {
          s.idsplit = want;
          s.id_next += want;
        } else {
          // What the range still holds is used first and the new range begins in mid-level: a level that dropped the rest of
          // its range (a third of the first range, on a scene of many small clusters) cost more ids than the reserve has to
          // spare (bvh_build_layout), and a tree that fits was declined.
          // The first range is what ANY tree over these points needs (leaves hold at most leaf_size points: at least
          // len / leaf_size of them, twice as many nodes less the root's own id) and is used up to the last id; later ones
          // (a quarter of that) may leave a few ids unused at the subtree's end.  If the ids are nearly out, the exact count
          // is asked for.
          const int need = want - have;
          const int sure = 2 * (len / leaf_size) - 2;
          int range = s.id_end == 0 ? sure : (sure / 4) & ~1;
          range = range > need ? range : need;
          int first = range > need ? try_alloc_nodes(a, range) : -1;
          if (first < 0) {
            range = need;
            first = alloc_nodes(a, need);
          }
          if (first < 0) {
            s.idbase = -1;
          } else {
            s.idsplit = have;
            s.idbase2 = first;
            s.id_next = first + need;
            s.id_end = first + range;
          }
        }
      }
      __syncthreads();
      const LevelIds ids{s.idbase, s.idsplit, s.idbase2};
      if (ids.base < 0) break;
      nint += nc;
      ++nlev;
      const int depth = root_depth + nlev - 1;  // of this level's nodes (nlev counts this level already)
      if (nc == 1) nodes_by_groups<kSubWaves>(a, s, b, cur, nc, ids, tid, leaf_size, depth);
      else if (nc == 2) nodes_by_groups<kSubWaves / 2>(a, s, b, cur, nc, ids, tid, leaf_size, depth);
      else if (nc <= 4) nodes_by_groups<kSubWaves / 4>(a, s, b, cur, nc, ids, tid, leaf_size, depth);
      else
        for (int e = wave; e < nc; e += kSubWaves)  // a wave per node
          node_in_lds(a, s, b, s.lb[cur][e], s.ll[cur][e], s.lg[cur][e], ids.pair_first(e), lane, cur ^ 1, leaf_size, depth);
      __syncthreads();
      if (tid == 0) s.lcount[cur] = 0;
      cur ^= 1;
      __syncthreads();
      if (nlev == 1) NB_STAMP(1)
      if (nlev == 2) NB_STAMP(2)
      if (nlev == 3) NB_STAMP(3)
    }
    // A subtree that stopped early (no ids left, or degenerate input: the fallback flag is up) leaves the nodes of `cur` unsplit
    // and unlisted.  Neither leaves nor parents, nobody below gives them a size, but the upward passes and the numbering add
    // their sizes up: one node each, not what an earlier build left in the record.
    for (int e = tid; e < s.lcount[cur]; e += kSubWaves * 64) a.nsize[s.lg[cur][e]] = 1;
    if (tid == 0) {
      s.loff[nlev] = nint;
      if (s.depth_max > 0) atomicMax(&a.flags[kBvhMaxDepth], s.depth_max);
    }
    __syncthreads();
    NB_STAMP(4)
    // leaves: children of the listed nodes that were not split further; a lane each, points still in LDS
    // (make_leaf :40-54, leaf mass and centre :98-131)
    for (int task = tid; task < 2 * nint; task += kSubWaves * 64) {
      const int c0 = a.nchild[list[task >> 1]];
      if (c0 < 0) continue;
      const int c = c0 + (task & 1);
      if (!a.nleaf[c]) continue;
      const int lb = a.nbegin[c] - b, ln = a.nlen[c];
      Box box;
      float sx = 0.f, sy = 0.f;
      uint32_t ms = 0u;
      for (int k = 0; k < ln; ++k) {  // slice order
        const float2 q = s.P[lb + k];
        box.add(q);
        sx = sx + q.x;
        sy = sy + q.y;
        ms += s.W[s.I[lb + k]];  // u32, wraps like the release build
      }
      a.nbox[c] = make_float4(box.mnx, box.mny, box.mxx, box.mxy);
      a.ncog[c] = make_float2(sx / (float)ln, sy / (float)ln);  // NaN for an empty leaf, as upstream
      a.nmass[c] = ms;
      a.nsize[c] = 1;
    }
    __syncthreads();
    NB_STAMP(5)
    // upward pass inside the subtree: deepest level first
    for (int lev = nlev - 1; lev >= 0; --lev) {
      for (int e = s.loff[lev] + tid; e < s.loff[lev + 1]; e += kSubWaves * 64) combine_children(a, list[e]);
      __syncthreads();
    }
    NB_STAMP(6)
    // the subtree's rows go back in their final order
    uint32_t ids[kSub / (kSubWaves * 64)];
#pragma unroll
    for (int j = 0; j < kSub / (kSubWaves * 64); ++j) {
      const int i = tid + j * kSubWaves * 64;
      ids[j] = i < len ? a.ID[b + s.I[i]] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSub / (kSubWaves * 64); ++j) {
      const int i = tid + j * kSubWaves * 64;
      if (i < len) {
        a.ID[b + i] = ids[j];
        a.P[b + i] = s.P[i];
      }
    }
    __syncthreads();
    NB_STAMP(7)
  }
}

}  // namespace

void launch_bvh_subtrees(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gs, const uint32_t* weight, int leaf_size,
                         int sub_start) {
  bvh_subtrees<<<dim3((unsigned)gs), dim3(kSubWaves * 64), 0, s>>>(make_ptrs(scratch, L), weight, leaf_size, sub_start);
}

}  // namespace nbody
