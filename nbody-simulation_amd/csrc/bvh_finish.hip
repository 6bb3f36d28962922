// The end of the device-side BVH build (f32, design: bvh_build.hip): the leaves and the upward pass above the subtrees
// (bvh_top_upward), then the pre-order numbering and the final arrays (bvh_emit; bvh_emit_gather with the step's row gather).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_device.h"
#include "bvh_units.h"

namespace nbody {

namespace {

__device__ __forceinline__ float lane_value(float v, int k) {  // k uniform
  return xsum::from_bits<float>((uint32_t)__builtin_amdgcn_readlane((int)xsum::to_bits(v), k));
}

// make_leaf (:40-54) + leaf mass and centre (:98-131) by one wave.  P: the leaf's points; wid(i): row of point i.
template <class PosPtr, class RowOf>
__device__ __forceinline__ void leaf_by_wave(const BvhPtrs& a, int leaf, PosPtr P, int len, int lane, const uint32_t* weight,
                                             RowOf row_of) {
  float mnx = kMaxF, mny = kMaxF, mxx = 0.f, mxy = 0.f, sx = 0.f, sy = 0.f;
  uint32_t ms = 0u;
  for (int k0 = 0; k0 < len; k0 += 64) {
    const int cnt = len - k0 < 64 ? len - k0 : 64;
    float2 q = make_float2(0.f, 0.f);
    if (lane < cnt) {
      q = P[k0 + lane];
      mnx = sse_min(mnx, q.x); mny = sse_min(mny, q.y);
      mxx = sse_max(mxx, q.x); mxy = sse_max(mxy, q.y);
      ms += weight[row_of(k0 + lane)];  // u32, wraps like the release build; any order
    }
    for (int k = 0; k < cnt; ++k) {  // slice order
      sx = sx + lane_value(q.x, k);
      sy = sy + lane_value(q.y, k);
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    mnx = sse_min(mnx, __shfl_xor(mnx, d, 64)); mny = sse_min(mny, __shfl_xor(mny, d, 64));
    mxx = sse_max(mxx, __shfl_xor(mxx, d, 64)); mxy = sse_max(mxy, __shfl_xor(mxy, d, 64));
    ms += (uint32_t)__shfl_xor((int)ms, d, 64);
  }
  if (lane == 0) {
    a.nbox[leaf] = make_float4(mnx, mny, mxx, mxy);
    a.ncog[leaf] = make_float2(sx / (float)len, sy / (float)len);  // NaN for an empty leaf, as upstream
    a.nmass[leaf] = ms;
    a.nsize[leaf] = 1;
  }
}

// The nodes above the subtrees (topq): leaves hanging directly off a long node, then the long nodes themselves,
// deepest level first.  One work-group: a few hundred nodes (a few thousand at N = 4M).
__global__ __launch_bounds__(256) void bvh_top_upward(BvhPtrs a, const uint32_t* __restrict__ weight) {
  constexpr int kKeep = 4096;       // entries whose (id, depth) stay in LDS; more than that are read again every level
  __shared__ int s_id[kKeep];
  __shared__ int16_t s_depth[kKeep];  // depth of a long internal node, -1: not one (a leaf, a subtree root)
  constexpr int kLeafList = 1024;
  __shared__ int s_dmax, s_nleaf;
  __shared__ int s_leaf[kLeafList];
  __shared__ int s_first[kBvhLevels + 2];  // where the entries of each depth begin: the levels append theirs one after the
                                           // other, so topq is ordered by depth and a level's loop visits its own range only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (a declined build goes on drawing slots for the children it could not make, bvh_big_count: topq holds a.cap entries)
  const int n_top = a.flags[kBvhTopCount] < a.cap ? a.flags[kBvhTopCount] : a.cap;
  if (tid == 0) { a.flags[kBvhBadIndex] = 0; s_dmax = -1; s_nleaf = 0; }
  for (int d = tid; d < kBvhLevels + 2; d += 256) s_first[d] = n_top;
  __syncthreads();
  // what each entry is, once (all threads side by side): the loops below visit every entry, the level loops at every depth
  const auto describe = [&](int e, int& id) {  // depth of a long internal node, -2 a leaf, -1 a subtree's root
    id = a.topq[e];
    if (a.nleaf[id]) return -2;
    return a.nlen[id] > kSub ? a.ndepth[id] : -1;
  };
  int dmax = -1;
  for (int e = tid; e < n_top; e += 256) {
    int id;
    const int d = describe(e, id);
    if (e < kKeep) { s_id[e] = id; s_depth[e] = (int16_t)d; }
    dmax = d > dmax ? d : dmax;
    int td = a.ndepth[id];
    td = td < 0 ? 0 : (td > kBvhLevels ? kBvhLevels : td);
    atomicMin(&s_first[td], e);
    if (d == -2) {  // a leaf hanging directly off a long node (few): listed, so that the waves below do not search for them
      const int slot = atomicAdd(&s_nleaf, 1);
      if (slot < kLeafList) s_leaf[slot] = e;
    }
  }
  if (dmax >= 0) atomicMax(&s_dmax, dmax);
  __syncthreads();
  if (tid == 0)  // a depth without entries begins where the next one does
    for (int d = kBvhLevels; d >= 0; --d) s_first[d] = s_first[d] < s_first[d + 1] ? s_first[d] : s_first[d + 1];
  __syncthreads();
  const bool listed = s_nleaf <= kLeafList;
  for (int k = wave; k < (listed ? s_nleaf : n_top); k += 4) {  // leaves hanging directly off a long node: a wave each
    const int e = listed ? s_leaf[k] : k;
    int id;
    const int kind = e < kKeep ? (id = s_id[e], (int)s_depth[e]) : describe(e, id);
    if (kind != -2) continue;
    const int b = a.nbegin[id];
    const uint32_t* ids = a.ID + b;
    leaf_by_wave(a, id, (const float2*)(a.P + b), a.nlen[id], lane, weight, [&](int i) { return ids[i]; });
  }
  __syncthreads();
  dmax = s_dmax;  // deepest long node: the tree below it belongs to the subtrees
  const auto entry = [&](int e, int& id) {
    if (e < kKeep) { id = s_id[e]; return (int)s_depth[e]; }
    return describe(e, id);
  };
  for (int d = dmax; d >= 0; --d) {
    for (int e = s_first[d] + tid; e < s_first[d + 1]; e += 256) {
      int id;
      if (entry(e, id) == d) combine_children(a, id);
    }
    __syncthreads();
  }
  if (tid == 0) a.flags[kBvhNodes] = a.nsize[0];  // the root's subtree: every node of the tree
  // pre-order numbers, top down: a node, its left subtree, its right subtree (the root has number 0); the nodes inside the
  // subtrees find theirs from here in bvh_emit
  for (int d = 0; d <= dmax; ++d) {
    for (int e = s_first[d] + tid; e < s_first[d + 1]; e += 256) {
      int id;
      if (entry(e, id) == d) {
        const int c0 = a.nchild[id];
        if (c0 >= 0) {
          a.npre[c0] = a.npre[id] + 1;
          a.npre[c0 + 1] = a.npre[id] + 1 + a.nsize[c0];
        }
      }
    }
    __syncthreads();
  }
}

// ---- numbering -----------------------------------------------------------------------------------------------------
// Final arrays in pre-order.  A node's number: walk up to the nearest ancestor whose number is known (one of the nodes above
// the subtrees), adding 1 per step and the left sibling's subtree where the step comes from a right child.
__device__ __forceinline__ void emit_node(const BvhPtrs& a, const int i, float4* __restrict__ geom0, float4* __restrict__ geom1,
                                          int4* __restrict__ link, int* __restrict__ depth_out, uint32_t* __restrict__ mass_out,
                                          float2* __restrict__ size_out) {
  const int ids = a.flags[kBvhNodeCount] < a.cap ? a.flags[kBvhNodeCount] : a.cap;  // ids handed out: not all are nodes
  const int m = a.flags[kBvhNodes];
  if (i >= ids || a.ndepth[i] < 0) return;
  int idx = 0, v = i;
  for (int guard = 0; a.npre[v] < 0 && guard <= kBvhLevels; ++guard) {
    const int p = a.nparent[v];
    const int c0 = a.nchild[p];
    idx += 1 + (v == c0 ? 0 : a.nsize[c0]);
    v = p;
  }
  // (this kernel also runs, blind, on trees whose long nodes are not all split yet: never write through a bad index)
  if (a.npre[v] < 0) {
    a.flags[kBvhBadIndex] = 1;
    return;
  }
  idx += a.npre[v];
  // (m is the root's subtree size: on a declined build a sum over whatever was made, not a bound on the arrays — a.cap is)
  if (idx < 0 || idx >= m || idx >= a.cap) {
    a.flags[kBvhBadIndex] = 1;
    return;
  }
  const int d = a.ndepth[i];
  const float4 box = a.nbox[i];
  const float w = box.z - box.x, h = box.w - box.y;  // boundary.size = max - min (:63-66)
  const float2 cog = a.ncog[i];
  const uint32_t ms = a.nmass[i];
  const float tx = sse_max(w, h), ty = sse_max(h, w);  // size.max(size.yx()), main.rs:371
  geom0[idx] = make_float4(box.x, box.y, box.x + w, box.y + h);
  geom1[idx] = make_float4(cog.x, cog.y, (float)ms, tx * ty);
  link[idx] = make_int4(idx + a.nsize[i], a.nbegin[i], a.nlen[i], a.nleaf[i]);  // skip: the first node after the subtree
  depth_out[idx] = d;
  mass_out[idx] = ms;
  size_out[idx] = make_float2(w, h);
}
__global__ __launch_bounds__(256) void bvh_emit(BvhPtrs a, float4* __restrict__ geom0, float4* __restrict__ geom1, int4* __restrict__ link,
                                                int* __restrict__ depth_out, uint32_t* __restrict__ mass_out,
                                                float2* __restrict__ size_out) {
  emit_node(a, (int)(blockIdx.x * 256 + threadIdx.x), geom0, geom1, link, depth_out, mass_out, size_out);
}
// bvh_emit and the row gather that follows it in every step (gather_particles) as ONE launch: two index spaces that do not depend
// on each other (the gather reads the permutation the partition left, not the numbering).  The numbering's work-groups come first:
// theirs is the longer chain (a walk up to the nearest numbered ancestor).  One launch of ~5 us less per step.
__global__ __launch_bounds__(256) void bvh_emit_gather(BvhPtrs a, float4* __restrict__ geom0, float4* __restrict__ geom1, int4* __restrict__ link,
                                                       int* __restrict__ depth_out, uint32_t* __restrict__ mass_out,
                                                       float2* __restrict__ size_out, const unsigned emit_groups, const GatherArgs<float> g) {
  if (blockIdx.x < emit_groups) emit_node(a, (int)(blockIdx.x * 256 + threadIdx.x), geom0, geom1, link, depth_out, mass_out, size_out);
  else gather_row<float>(g, (int64_t)(blockIdx.x - emit_groups) * 256 + threadIdx.x);
}

}  // namespace

void launch_bvh_top_upward(hipStream_t s, char* scratch, const BvhBuildLayout& L, const uint32_t* weight) {
  bvh_top_upward<<<dim3(1), dim3(256), 0, s>>>(make_ptrs(scratch, L), weight);
}
void launch_bvh_emit(hipStream_t s, char* scratch, const BvhBuildLayout& L, dim3 gm, void* geom0, void* geom1, void* link,
                     int* depth_out, uint32_t* mass_out, float2* size_out) {
  bvh_emit<<<gm, dim3(256), 0, s>>>(make_ptrs(scratch, L), (float4*)geom0, (float4*)geom1, (int4*)link, depth_out, mass_out, size_out);
}
void launch_bvh_emit_gather(hipStream_t s, char* scratch, const BvhBuildLayout& L, dim3 gm, void* geom0, void* geom1, void* link,
                            int* depth_out, uint32_t* mass_out, float2* size_out, const GatherArgs<float>& gather) {
  const unsigned gg = (unsigned)((gather.n + 255) / 256);
  bvh_emit_gather<<<dim3(gm.x + gg), dim3(256), 0, s>>>(make_ptrs(scratch, L), (float4*)geom0, (float4*)geom1, (int4*)link, depth_out, mass_out, size_out, gm.x,
                                                        gather);
}

}  // namespace nbody
