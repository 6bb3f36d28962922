// The retired designs of the big-leaf BVH walk, kept for A/B runs: laboratory build only (the product's object of this unit holds
// no device code).  The three-pass walk of round 1, the breadth-first FAST walk and the chunk ordering of round 4, and the
// per-wave log of the FAST register walk (development).
#ifdef NBODY_LAB
// ---- the three-pass walk of round 1 (count / emit terms / sum) --------------------------------------------------------------
// The Barnes-Hut walk in three passes — same nodes, same pairs, same operations, same order of additions as the fused
// walk (tree_kernels.hip) and the CPU recursion (the reference's src/main.rs:348-386), so still bit-identical — for
// trees with big leaves (the BVH: up to 64 particles per leaf), f32.
//
// Why: in the fused walk a wave that reaches a leaf evaluates the leaf's particles one after the other for all of
// its lanes at once, ~56 instructions per particle (two IEEE divisions) whether 3 or 60 lanes take part; the targets
// near the reference scene's heavy bodies visit 20x the median number of leaves, their waves run 1.2 ms while most of
// the chip idles.  The only thing that has to be sequential is the ADDITION of a target's terms; their values do not
// depend on one another.  So:
//   1. walk_count: the traversal alone (node tests, no arithmetic): how many terms does each target have;
//      an exclusive scan turns the counts into offsets into one big term array (HBM is 288 GB: ~250 MB here);
//   2. walk_terms: the traversal again; an accepted node writes its term; at a leaf the wave takes its acting lanes
//      one at a time and all 64 lanes evaluate that target against 64 particles of the leaf at once (lane = particle),
//      so the cost of a leaf step is proportional to the lanes that want it, and nothing is summed;
//      a pair the reference skips (|dx|+|dy| not normal, main.rs:241-243) writes -0.0, the identity of IEEE addition;
//   3. walk_sum: per target, the terms are added in order from +0.0 — one v_add_f32_dpp per term and coordinate, a row of
//      16 lanes per target.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <cstdio>
#include <vector>

#include "env.h"
#include "walk_arms.h"
#include "walk_device.h"
#include "walk_split.h"

namespace nbody {

namespace {

// The traversal both passes share.  F: what to do with an accepted node / a leaf.
template <bool EMIT, int kTPW, bool FAST>
__global__ __launch_bounds__(256) void walk_pass(const WalkArgs<float> a, uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                 float2* __restrict__ terms, const int* __restrict__ info, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (EMIT && (info[1] != 0)) return;  // the term array is too small: the caller grows it
  int64_t t;
  bool live;
  if (EMIT) {
    // Waves by WORK, not by head count: wave w takes the targets t with g(t) = off[t] / budget + t / 64 == w
    // (g never decreases: at most 64 targets, about `budget` terms — a target with thousands of terms walks alone,
    // and its wave is as short as its own path).  The two ends of the range by binary search.
    const uint32_t budget = (uint32_t)info[3];  // set by walk_total
    int64_t lo = 0, hi = a.n_tgt;
    while (lo < hi) {  // first t with g(t) >= wave
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)(off[mid] / budget) + (mid >> 6) < wave) lo = mid + 1; else hi = mid;
    }
    const int64_t t0 = lo;
    hi = t0 + 64 < a.n_tgt ? t0 + 64 : a.n_tgt;
    while (lo < hi) {  // first t with g(t) > wave
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)(off[mid] / budget) + (mid >> 6) <= wave) lo = mid + 1; else hi = mid;
    }
    if (lo == t0) return;  // no target has this number
    t = t0 + lane;
    live = t < lo;
  } else {
    t = wave * kTPW + lane;
    live = lane < kTPW && t < a.n_tgt;
  }
  const int64_t row = live ? (a.tgt_index ? (int64_t)a.tgt_index[t] : t) : 0;
  const float2 p = live ? reinterpret_cast<const float2*>(a.tgt_pos)[row] : make_float2(0.f, 0.f);
  const float4* __restrict__ g0 = reinterpret_cast<const float4*>(a.geom0);
  const float4* __restrict__ g1 = reinterpret_cast<const float4*>(a.geom1);
  const int4* __restrict__ lk = reinterpret_cast<const int4*>(a.link);
  const float2* __restrict__ lpos = reinterpret_cast<const float2*>(a.leaf_pos);
  const float* __restrict__ lmass = a.leaf_mass;
  const float theta = a.theta, clamp = a.clamp;
  const int n_nodes = a.n_nodes;
  int resume = live ? 0 : n_nodes;
  uint32_t n_terms = 0;                       // terms of this lane's target so far
  const uint32_t base = (EMIT && live) ? off[t] : 0u;
  int i = 0;
#ifdef NB_WALK_TIMING
  long long tw0 = wall_clock64(), t_leaf = 0, t_node = 0;
#endif
  while (i < n_nodes) {  // i is wave-uniform
#ifdef NB_WALK_TIMING
    const long long ts = wall_clock64();
#endif
    const int4 l = lk[i];    // the three records of a node are fetched together: one latency per step, not two
    const float4 b = g0[i];  // lo.x lo.y hi.x hi.y
    const float4 c = g1[i];  // cog.x cog.y mass s2
    const bool act = resume <= i;
    int next;
    if (l.w) {  // Leaf arm, main.rs:351-363: every particle of the slice, in slice order
      if (EMIT) {
        unsigned long long mask = __builtin_amdgcn_ballot_w64(act);
        for (int k0 = 0; k0 < l.z; k0 += 64) {  // 64 particles at a time, lane = particle
          const int mine = k0 + lane;
          float2 q = make_float2(0.f, 0.f);
          float m = 0.f;
          if (mine < l.z) {
            q = lpos[l.y + mine];
            m = lmass[l.y + mine];
          }
          unsigned long long todo = mask;
          while (todo) {  // one acting target after the other
            const int tl = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float tx = lane_f(p.x, tl), ty = lane_f(p.y, tl);
            const uint32_t dst = (uint32_t)__builtin_amdgcn_readlane((int)(base + n_terms), tl) + (uint32_t)k0;
            if (mine < l.z) terms[dst + lane] = term_of<FAST>(tx, ty, q.x, q.y, m, clamp);
          }
        }
      }
      if (act) {
        n_terms += (uint32_t)l.z;
        resume = l.x;
      }
      next = l.x;
    } else {
      bool descend = false;
      if (act) {
        const bool contains = p.y > b.y && p.x > b.x && p.x < b.z && p.y < b.w;  // bvh_tree.rs:15-20 (all strict)
        const float ddx = p.x - c.x, ddy = p.y - c.y;                              // dist2(p, cog), main.rs:228-232
        const float d2 = ddx * ddx + ddy * ddy;
        if (!contains && c.w < d2 * theta * theta) {                               // :370-372
          if (EMIT) terms[base + n_terms] = term_of<FAST>(p.x, p.y, c.x, c.y, c.z, clamp);  // :374-379
          ++n_terms;
          resume = l.x;
        } else {
          descend = true;                                                          // :381-382
          resume = i + 1;
        }
      }
      next = __builtin_amdgcn_ballot_w64(descend) != 0 ? i + 1 : l.x;
    }
    i = __builtin_amdgcn_readfirstlane(next);
#ifdef NB_WALK_TIMING
    if (l.w) t_leaf += wall_clock64() - ts; else t_node += wall_clock64() - ts;
#endif
  }
#ifdef NB_WALK_TIMING
  if (EMIT && lane == 0) {  // longest wave: total us << 20 | leaf us << 10 | node us
    const long long tot = wall_clock64() - tw0;
    atomicMax(const_cast<int*>(info) + 5, (int)(((tot / 100) << 20) | (((t_leaf / 100) & 1023) << 10) | ((t_node / 100) & 1023)));
  }
#endif
  if (!EMIT && live) cnt[t] = n_terms;
}

// total = off[n-1] + cnt[n-1]; flag what does not fit
__global__ void walk_total(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, int64_t n, int64_t capacity,
                           int* __restrict__ info) {
  const unsigned long long total = n > 0 ? (unsigned long long)off[n - 1] + cnt[n - 1] : 0ull;
  // (the scan is 32 bits wide: walk_check_wrap has flagged a wrapped sum already)
  info[0] = (int)(total > 0x7fffffffull ? 0x7fffffffull : total);
  if (total > (unsigned long long)capacity) info[1] = 1;
  // the term pass' budget per wave: enough for a dozen average targets (each wave repeats the traversal: where every
  // target is heavy, few targets per wave only multiply that), never less than kTermBudget; a power of two
  unsigned long long want = n > 0 ? kBudgetTargets * total / (unsigned long long)n : 0ull;
  uint32_t budget = kTermBudget;
  while (budget < want && budget < (1u << 30)) budget <<= 1;
  info[3] = (int)budget;
}

template <int K> __device__ __forceinline__ void add_row_lane(float& s, float v) {
  asm volatile("v_add_f32_dpp %0, %1, %0 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(s) : "v"(v), "n"(K));
}

// acc[target] = ((+0 + t0) + t1) + ... in order; a row of 16 lanes per target, 16 terms per round.
__global__ __launch_bounds__(256) void walk_sum(const WalkArgs<float> a, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                const float2* __restrict__ terms, const int* __restrict__ info) {
  if (info[1] != 0) return;
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const int64_t t = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const bool live = t < a.n_tgt;
  const uint32_t n = live ? cnt[t] : 0u;
  const uint32_t base = live ? off[t] : 0u;
  uint32_t nmax = n;  // the wave runs as long as its longest target
  for (int d = 32; d >= 16; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)nmax, d, 64);
    nmax = o > nmax ? o : nmax;
  }
  float sx = 0.f, sy = 0.f;  // Vec2::zero(), main.rs:409
  // 256 terms per round: sixteen loads in flight per lane, then 512 dependent adds (16 terms add in ~0.06 us, a
  // load takes ~2 us: the longest target, not the bandwidth, sets this kernel's time)
  constexpr int R = 16;
  for (uint32_t p = 0; p < nmax; p += 16 * R) {
    float2 q[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t k = p + 16u * j + (uint32_t)sub;
      q[j] = k < n ? terms[base + k] : make_float2(-0.0f, -0.0f);  // past the end: the identity of addition
    }
    asm volatile("s_nop 1" ::: "memory");  // q may come from a VALU move: 2 wait states before a DPP read
#define NB_ADD(K) add_row_lane<K>(sx, q[j].x); add_row_lane<K>(sy, q[j].y);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      NB_ADD(0) NB_ADD(1) NB_ADD(2) NB_ADD(3) NB_ADD(4) NB_ADD(5) NB_ADD(6) NB_ADD(7)
      NB_ADD(8) NB_ADD(9) NB_ADD(10) NB_ADD(11) NB_ADD(12) NB_ADD(13) NB_ADD(14) NB_ADD(15)
    }
#undef NB_ADD
  }
  if (live && sub == 0) {
    const int64_t row = a.tgt_index ? (int64_t)a.tgt_index[t] : t;
    reinterpret_cast<float2*>(a.acc)[row] = make_float2(sx, sy);
  }
}

// the first target t with g(t) >= wave (n_tgt if none): the whole wave calls it
[[maybe_unused]] __device__ __forceinline__ int first_target_reaching(const uint32_t* __restrict__ off, const int n_tgt, const int wave, const uint32_t M, const int lane) {
  int lo = 0, hi = n_tgt;
  while (lo < hi) {
    const int step = (hi - lo + 63) >> 6;
    const int idx = lo + lane * step;
    const bool reached = idx >= hi || off_quot(off[idx], M) + (idx >> 6) >= wave;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(reached);
    const int first = m ? __builtin_ctzll(m) : 64;
    if (first == 0) { hi = lo; break; }
    const int below = lo + (first - 1) * step;
    if (first < 64) hi = min(hi, lo + first * step);
    lo = below + 1;
  }
  return lo;
}

// ---- the FAST one-pass walk, BREADTH FIRST (round 4) ------------------------------------------------------------------
// walk_tile_fast (walk_tile_fast.hip) is its longest wave's serial chain (profiles/r03_walk_fast_variants.txt: 0.355 us per node step — a scalar
// load's round trip plus ~100 dependent instructions — 414 node steps in the reference scene's longest wave, 273 of the kernel's
// 334 us).  The depth-first order is what makes it a chain: node i's record must arrive before anyone knows which record comes
// next.  Under the tolerance contract the ORDER of a target's terms is free, and the traversal itself never needed it: a lane acts
// at a node iff it descended through the parent, so a node's acting lanes are its parent's descend mask.  So the wave keeps a
// DEQUE of (node, 64-bit lane mask) in LDS and takes up to 64 entries at a time from its head (breadth first): 64 lanes fetch 64
// nodes' records — and the right siblings' indices, link[i + 1].x — in ONE round trip, then the entries are tested one after the
// other with the record broadcast out of registers (v_readlane: SGPR operands, no memory in the loop); accepted nodes' terms are
// taken on the spot, leaves (and three-node subtrees, as in the depth-first walk) go to a small list that is worked off after the
// batch, the next leaf's particles on their way while this one's rounds run.  Same node tests, same interaction lists, same
// terms as walk_tile_fast (nbody_tree_walk_stats and the history are unchanged); only the order of additions differs, and it is
// a fixed function of the inputs (no atomics): bitwise reproducible.
// MEASURED (profiles/r04_walk_bfs_ab.txt): correct (every FAST parity test green) and SLOWER — 0.579 against 0.338 ms on the
// reference scene, 4.96 against 2.99 ms at Plummer 1 M.  The union of a wave's paths is NARROW: its 64 tree-contiguous targets
// share one chain from the root to their region, so a level holds ~4 entries, not ~64, and every level pays a vector load's round
// trip (longer than the scalar load's it replaces) plus the deque's hand-offs, at 5 waves per SIMD instead of 8 (28 KB of LDS
// per group, 81 VGPRs).  Laboratory build only (NBODY_WALK_FAST_BFS=1); the product walks depth first.
// The deque cannot outgrow its LDS: while it is nearly full the wave takes ONE entry from the TAIL instead (depth first: a
// stack grows by at most the depth of the subtree it is in, and the device builds stop at 56 levels); should it still fill
// up, the overflow word is set and the caller gets an error instead of a wrong answer.
constexpr int kBfsQ = 512;          // deque slots per wave (12 B each)
constexpr int kBfsHeadroom = 192;   // breadth first only while at least this many slots are free
constexpr int kBfsLeaves = 64;      // leaf entries per batch: one per entry taken

__device__ __forceinline__ int rl(int v, int lane_sel) { return __builtin_amdgcn_readlane(v, lane_sel); }
__device__ __forceinline__ float rlf(float v, int lane_sel) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane_sel)); }

// One leaf step of the FAST walk for the lanes of `mask` (`act`: this lane is one of them) against the particles [first, first +
// count): walk_tile_fast's rounds (lane = particle, eight targets' rows reduced together; lane = target where most of the wave
// wants the leaf).  (q0, m0): the first 64 particles, already fetched by the caller.
template <class T>
__device__ __forceinline__ void fast_leaf_step(const unsigned long long mask, const bool act, const int first, const int count, const int lane,
                                               const typename Vec2Of<T>::type p, const T clamp, const typename Vec2Of<T>::type* __restrict__ lpos,
                                               const T* __restrict__ lmass, typename Vec2Of<T>::type q0, T m0, T& bx, T& by) {
  using T2 = typename Vec2Of<T>::type;
  const int takers = __builtin_popcountll(mask);
  const int rank = act ? (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u)) : -1;
  for (int k0 = 0; k0 < count; k0 += 64) {  // 64 particles at a time
    const int mine = k0 + lane;
    const int left = count - k0;
    const int mc = left < 64 ? left : 64;
    T2 q = q0;
    T m = m0;
    if (k0 > 0) {
      q = T2{0, 0};
      m = 0;  // a lane past the end: force 0, its terms are exact zeros
      if (mine < count) {
        q = lpos[first + mine];
        m = lmass[first + mine];
      }
    }
    if (takers * kFastRoundCost > mc * kFastPairCost) {  // most of the wave wants this leaf: lane = target
      for (int j = 0; j < mc; ++j) {
        const T qx = lane_t(q.x, j), qy = lane_t(q.y, j), qm = lane_t(m, j);
        if (act) {
          const T dx = qx - p.x, dy = qy - p.y;
          const T sc = fast_scale(dx, dy, qm, clamp);
          bx = fma_t(dx, sc, bx);
          by = fma_t(dy, sc, by);
        }
      }
      continue;
    }
    unsigned long long todo = mask;
    int batch0 = 0;
#define NB_FAST_ROUND(XV, YV)                                             \
  {                                                                       \
    const int tl = __builtin_ctzll(todo);                                 \
    todo &= todo - 1;                                                     \
    const T dx = q.x - lane_t(p.x, tl), dy = q.y - lane_t(p.y, tl);       \
    const T sc = fast_scale(dx, dy, m, clamp);                            \
    XV = dx * sc;                                                         \
    YV = dy * sc;                                                         \
  }
    while (todo) {
      const int left_t = takers - batch0;
      const int k = rank - batch0;  // this lane's place in the batch, if it is an acting target
      T gx, gy;
      int took;
      if (left_t > 4) {  // eight targets (missing ones contribute zeros): x and y reduced side by side
        T X[8], Y[8];
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) NB_FAST_ROUND(X[sl], Y[sl])
#pragma unroll
        for (int sl = 5; sl < 8; ++sl) {
          X[sl] = 0;
          Y[sl] = 0;
          if (todo) NB_FAST_ROUND(X[sl], Y[sl])
        }
        const T rx = reduce8(X), ry = reduce8(Y);
        const int src = slot_lane8(k & 7);
        gx = lane_fetch(rx, src);
        gy = lane_fetch(ry, src);
        took = 8;
      } else if (left_t > 2) {  // three or four targets: their x and y are the eight values of ONE reduction
        T V[8];
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) NB_FAST_ROUND(V[2 * sl], V[2 * sl + 1])
        V[6] = 0;
        V[7] = 0;
        if (todo) NB_FAST_ROUND(V[6], V[7])
        const T r = reduce8(V);
        const int src = 16 * (k & 1) + 8 * ((k >> 1) & 1);
        gx = lane_fetch(r, src);
        gy = lane_fetch(r, src + 32);
        took = 4;
      } else if (left_t == 2) {  // two targets: four values
        T V[4];
        NB_FAST_ROUND(V[0], V[1])
        NB_FAST_ROUND(V[2], V[3])
        const T r = reduce4(V);
        const int src = 16 * (k & 1);
        gx = lane_fetch(r, src);
        gy = lane_fetch(r, src + 32);
        took = 2;
      } else {  // one target
        T x, y;
        NB_FAST_ROUND(x, y)
        const T r = reduce2(x, y);
        gx = lane_t(r, 16);
        gy = lane_t(r, 48);
        took = 1;
      }
      if (k >= 0 && k < took) {
        bx = bx + gx;
        by = by + gy;
      }
      batch0 += took;
    }
#undef NB_FAST_ROUND
  }
}

__global__ __launch_bounds__(256) void walk_tile_fast_bfs(const WalkArgs<float> a, const uint32_t* __restrict__ off, int* __restrict__ info,
                                                          const uint32_t* __restrict__ tgt_ids, uint32_t* __restrict__ hist,
                                                          unsigned long long* __restrict__ total_out) {
  __shared__ int q_idx_all[4][kBfsQ];
  __shared__ unsigned q_lo_all[4][kBfsQ], q_hi_all[4][kBfsQ];
  __shared__ int lf_first_all[4][kBfsLeaves], lf_count_all[4][kBfsLeaves];
  __shared__ unsigned lf_lo_all[4][kBfsLeaves], lf_hi_all[4][kBfsLeaves];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  int* __restrict__ q_idx = q_idx_all[wib];
  unsigned* __restrict__ q_lo = q_lo_all[wib];
  unsigned* __restrict__ q_hi = q_hi_all[wib];
  int* __restrict__ lf_first = lf_first_all[wib];
  int* __restrict__ lf_count = lf_count_all[wib];
  unsigned* __restrict__ lf_lo = lf_lo_all[wib];
  unsigned* __restrict__ lf_hi = lf_hi_all[wib];
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + wib));
  if (info[1] != 0) return;  // the estimate's scan wrapped: the caller walks again without one
  if (wave > info[5]) return;  // past the last wave that can hold a target
  const uint32_t qmul = 0xFFFFFFFFu / (uint32_t)__builtin_amdgcn_readfirstlane(info[3]);  // (budget >= 64)
  const int n_tgt = (int)a.n_tgt;
  int t0, lo;
  wave_targets(off, n_tgt, wave, qmul, lane, t0, lo);
  if (lo == t0) return;
  const int64_t t = (int64_t)t0 + lane;
  const bool live = t < lo;
  const int64_t row = live ? (a.tgt_index ? (int64_t)a.tgt_index[t] : t) : 0;
  const float2 p = live ? reinterpret_cast<const float2*>(a.tgt_pos)[row] : float2{0, 0};
  const float4* __restrict__ g0 = reinterpret_cast<const float4*>(a.geom0);
  const float4* __restrict__ g1 = reinterpret_cast<const float4*>(a.geom1);
  const int4* __restrict__ lk = reinterpret_cast<const int4*>(a.link);
  const float2* __restrict__ lpos = reinterpret_cast<const float2*>(a.leaf_pos);
  const float* __restrict__ lmass = a.leaf_mass;
  const float theta = a.theta, clamp = a.clamp;
  const int n_nodes = a.n_nodes_dev ? __builtin_amdgcn_readfirstlane(*a.n_nodes_dev) : a.n_nodes;
  uint32_t n_terms = 0;
  float ax = 0, ay = 0, bx = 0, by = 0;  // two-level summation, as walk_tile_fast: the block sum joins the total every fourth leaf step
  int leaf_steps = 0;
  const int last = n_nodes - 1;
  int head = 0, occ = 0;  // wave-uniform
  const unsigned long long live_mask = __builtin_amdgcn_ballot_w64(live);
  if (n_nodes > 0 && lane == 0) {
    q_idx[0] = 0;
    q_lo[0] = (unsigned)live_mask;
    q_hi[0] = (unsigned)(live_mask >> 32);
  }
  if (n_nodes > 0) occ = 1;
  bool overflow = false;
  while (occ > 0) {
    // ---- take a batch: from the head while there is room for its children (breadth first), else the newest entry alone
    int B, start;
    if (occ <= kBfsQ - kBfsHeadroom) {
      B = occ < 64 ? occ : 64;
      start = head;
      head = (head + B) & (kBfsQ - 1);
    } else {
      B = 1;
      start = (head + occ - 1) & (kBfsQ - 1);
    }
    occ -= B;
    wave_lds_handoff();  // the entries' stores (lane 0, the batch before) before these reads
    int my_idx = 0;
    unsigned my_lo = 0, my_hi = 0;
    if (lane < B) {
      const int pos = (start + lane) & (kBfsQ - 1);
      my_idx = q_idx[pos];
      my_lo = q_lo[pos];
      my_hi = q_hi[pos];
    }
    // ---- the batch's records, one round trip: link, box, centre of gravity | mass | s^2, and the right sibling's index
    my_idx = my_idx < last ? my_idx : last;
    const int4 ml = lk[my_idx];
    const float4 mb = g0[my_idx];
    const float4 mc = g1[my_idx];
    const int mr = lk[my_idx < last ? my_idx + 1 : last].x;  // skip of node i + 1 = node i's right child (inner nodes)
    int nleaf = 0;
    for (int e = 0; e < B; ++e) {
      const int i = rl(my_idx, e);
      const int lx = rl(ml.x, e), ly = rl(ml.y, e), lz = rl(ml.z, e), lw = rl(ml.w, e);
      const unsigned long long m = ((unsigned long long)(unsigned)rl((int)my_hi, e) << 32) | (unsigned)rl((int)my_lo, e);
      const bool act = (m >> lane) & 1ull;
      if (lw) {  // Leaf arm, main.rs:351-363
        if (lane == 0) {
          lf_first[nleaf] = ly;
          lf_count[nleaf] = lz;
          lf_lo[nleaf] = (unsigned)m;
          lf_hi[nleaf] = (unsigned)(m >> 32);
        }
        ++nleaf;
        n_terms += act ? (uint32_t)lz : 0u;
        continue;
      }
      const float b_x = rlf(mb.x, e), b_y = rlf(mb.y, e), b_z = rlf(mb.z, e), b_w = rlf(mb.w, e);
      const float c_x = rlf(mc.x, e), c_y = rlf(mc.y, e), c_z = rlf(mc.z, e), c_w = rlf(mc.w, e);
      // the node test is the exact walk's, bit for bit (bvh_tree.rs:15-20 all strict; main.rs:228-232, :370-372)
      const bool contains = (p.y > b_y) & (p.x > b_x) & (p.x < b_z) & (p.y < b_w);
      const float ddx = p.x - c_x, ddy = p.y - c_y;
      const float d2 = ddx * ddx + ddy * ddy;
      const bool accept = act & !contains & (c_w < d2 * theta * theta);
      const bool descend = act & !accept;
      const float dx = c_x - p.x, dy = c_y - p.y;  // :374-379
      const float sc = fast_scale(dx, dy, c_z, clamp);
      const float nbx = fma_t(dx, sc, bx), nby = fma_t(dy, sc, by);
      bx = accept ? nbx : bx;
      by = accept ? nby : by;
      n_terms += accept ? 1u : 0u;
      const unsigned long long dmask = __builtin_amdgcn_ballot_w64(descend);
      if (dmask == 0) continue;
      if (lx - i == 3) {  // both children are leaves: their particles are this node's own range (walk_tile_fast's three-node fold)
        if (lane == 0) {
          lf_first[nleaf] = ly;
          lf_count[nleaf] = lz;
          lf_lo[nleaf] = (unsigned)dmask;
          lf_hi[nleaf] = (unsigned)(dmask >> 32);
        }
        ++nleaf;
        n_terms += descend ? (uint32_t)lz : 0u;
        continue;
      }
      if (occ + 2 > kBfsQ) {  // never expected (see above): say so instead of walking on with a hole in the lists
        overflow = true;
        continue;
      }
      const int right = rl(mr, e);
      if (lane == 0) {
        const int t0q = (head + occ) & (kBfsQ - 1), t1q = (head + occ + 1) & (kBfsQ - 1);
        q_idx[t0q] = i + 1;  // children[0] then children[1], main.rs:381-382
        q_lo[t0q] = (unsigned)dmask;
        q_hi[t0q] = (unsigned)(dmask >> 32);
        q_idx[t1q] = right;
        q_lo[t1q] = (unsigned)dmask;
        q_hi[t1q] = (unsigned)(dmask >> 32);
      }
      occ += 2;
    }
    if (nleaf == 0) continue;
    // ---- the batch's leaves: the next one's particles are fetched while this one's rounds run
    wave_lds_handoff();
    int f_cur = lf_first[0], c_cur = lf_count[0];
    float2 q_cur = float2{0, 0};
    float m_cur = 0;
    if (lane < c_cur) {
      q_cur = lpos[f_cur + lane];
      m_cur = lmass[f_cur + lane];
    }
    for (int j = 0; j < nleaf; ++j) {
      const unsigned long long m = ((unsigned long long)lf_hi[j] << 32) | lf_lo[j];
      int f_nxt = 0, c_nxt = 0;
      float2 q_nxt = float2{0, 0};
      float m_nxt = 0;
      if (j + 1 < nleaf) {
        f_nxt = lf_first[j + 1];
        c_nxt = lf_count[j + 1];
        if (lane < c_nxt) {
          q_nxt = lpos[f_nxt + lane];
          m_nxt = lmass[f_nxt + lane];
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // (the loads above stay above the rounds below)
      fast_leaf_step<float>(m, (m >> lane) & 1ull, f_cur, c_cur, lane, p, clamp, lpos, lmass, q_cur, m_cur, bx, by);
      if (++leaf_steps == 4) {
        ax = ax + bx;
        ay = ay + by;
        bx = by = 0;
        leaf_steps = 0;
      }
      f_cur = f_nxt;
      c_cur = c_nxt;
      q_cur = q_nxt;
      m_cur = m_nxt;
    }
  }
  ax = ax + bx;
  ay = ay + by;
  if (overflow && lane == 0) info[1] = 1;
  if (live) {
    reinterpret_cast<float2*>(a.acc)[row] = float2{ax, ay};
    if (hist) hist[tgt_ids[t]] = n_terms;  // by particle id: the rows are permuted by every build
  }
  unsigned long long sum = live ? n_terms : 0ull;  // what this walk cost, for the next estimate's scale
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
  if (lane == 0) atomicAdd(total_out, sum);
}

// ---- which work-groups go first (round 4) --------------------------------------------------------------------------------
// On a scene whose waves do not all fit the chip at once (Plummer 1 M: 17 400 waves on 8 192 slots) the work-groups are
// dispatched in index order = tree order, and the dense centre's long waves (2.2 ms against a mean of 0.9) sit in the middle of
// it: those past the first residency round start a millisecond late and end the kernel at 2.9 ms where the sum of all wave
// times over the slots is 1.9 (profiles/r04_walk_wave_log.txt).  So the groups are dealt out longest first — in CHUNKS of
// consecutive groups (neighbouring groups walk neighbouring targets and share their nodes and leaves in the L2s: dealing single
// groups out costs 10-25 %), a chunk's weight being its targets' estimated terms, which the scan has left in `off`.  One
// work-group: a wave per chunk finds the chunk's first target (the walk's own 64-ary search), then the chunks are ranked.
// MEASURED (profiles/r04_walk_order_ab.txt): heaviest first gains 10 % at Plummer 1 M (f32) and 6-8 % at 655 360 / 1 M in f64, and LOSES
// 5 % at 655 360 and 4-8 % at 2 M in f32; "lightest last" gains nothing anywhere.  No rule follows from that, so the product keeps the
// index order and this stays a laboratory switch (NBODY_WALK_ORDER=2 / 1).
// mode 2: all chunks heaviest first.  mode 1: the LIGHTEST chunks — as many as one residency round holds — go last, everything else stays
// in index order: what matters is that no long wave starts late, and the rest of the order is the locality the walks live on.
__global__ __launch_bounds__(1024) void walk_order_chunks(const uint32_t* __restrict__ off, const int n_tgt, const int* __restrict__ info,
                                                         const int chunk_groups, const int n_chunks, int* __restrict__ order, const int mode,
                                                         const int n_light) {
  __shared__ int bnd[kWalkOrderChunks + 1];
  __shared__ unsigned long long cost[kWalkOrderChunks];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t M = 0xFFFFFFFFu / (uint32_t)__builtin_amdgcn_readfirstlane(info[3]);
  for (int c = w; c < n_chunks; c += 16) {
    const int t = first_target_reaching(off, n_tgt, c * chunk_groups * 4, M, lane);
    if (lane == 0) bnd[c] = t;
  }
  if (tid == 0) bnd[n_chunks] = n_tgt;
  __syncthreads();
  const unsigned long long total = (unsigned long long)(unsigned)info[0];
  if (tid < n_chunks) {
    const int b0 = bnd[tid], b1 = bnd[tid + 1];
    const unsigned long long o0 = b0 < n_tgt ? off[b0] : total, o1 = b1 < n_tgt ? off[b1] : total;
    // (the estimate's terms and, so that equal estimates still order by work, the head count)
    cost[tid] = (o1 >= o0 ? o1 - o0 : 0ull) + (unsigned long long)(b1 - b0);
  }
  __syncthreads();
  __shared__ unsigned char light[kWalkOrderChunks];
  int rank = 0;  // among all chunks, heaviest first (a bijection: every chunk has its own rank)
  if (tid < n_chunks) {
    const unsigned long long mine = cost[tid];
    for (int h = 0; h < n_chunks; ++h) rank += (cost[h] > mine || (cost[h] == mine && h < tid)) ? 1 : 0;
    light[tid] = rank >= n_chunks - n_light ? 1 : 0;
  }
  __syncthreads();
  if (tid < n_chunks) {
    if (mode == 2) {
      order[rank] = tid;
    } else {
      int before_same = 0;  // chunks of my kind before me, in index order
      for (int h = 0; h < tid; ++h) before_same += light[h] == light[tid] ? 1 : 0;
      order[light[tid] ? n_chunks - n_light + before_same : before_same] = tid;
    }
  }
}

}  // namespace

hipError_t launch_tree_walk_split(hipStream_t s, const WalkArgs<float>& a, char* scratch, const WalkSplitLayout& L, void* terms,
                                  int64_t term_capacity) {
  if (a.n_tgt <= 0) return hipSuccess;
  uint32_t* cnt = (uint32_t*)(scratch + L.cnt);
  uint32_t* off = (uint32_t*)(scratch + L.off);
  int* info = (int*)(scratch + L.info);
  const int64_t cwaves = (a.n_tgt + kCountTPW - 1) / kCountTPW;
  const int64_t twaves = term_capacity / kTermBudget + a.n_tgt / 64 + 2;  // upper bound of g(t) + 1
  hipError_t e = hipMemsetAsync(info, 0, 32, s);
  if (e != hipSuccess) return e;
  walk_pass<false, kCountTPW, false><<<dim3((unsigned)((cwaves + 3) / 4)), dim3(256), 0, s>>>(a, cnt, nullptr, nullptr, info, term_capacity);
  e = launch_walk_count_scan(s, scratch, L, a.n_tgt);
  if (e != hipSuccess) return e;
  walk_total<<<dim3(1), dim3(1), 0, s>>>(cnt, off, a.n_tgt, term_capacity, info);
  if (a.fast) walk_pass<true, 64, true><<<dim3((unsigned)((twaves + 3) / 4)), dim3(256), 0, s>>>(a, cnt, off, (float2*)terms, info, term_capacity);
  else walk_pass<true, 64, false><<<dim3((unsigned)((twaves + 3) / 4)), dim3(256), 0, s>>>(a, cnt, off, (float2*)terms, info, term_capacity);
  const int64_t sum_waves = (a.n_tgt + 3) / 4;
  walk_sum<<<dim3((unsigned)((sum_waves + 3) / 4)), dim3(256), 0, s>>>(a, cnt, off, (const float2*)terms, info);
  return hipGetLastError();
}

hipError_t launch_walk_tile_fast_bfs(const TileLaunch& k, const WalkArgs<float>& a) {
  walk_tile_fast_bfs<<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
  return hipGetLastError();
}

// more waves than the chip holds at once (256 CUs x 32): chunks of work-groups, heaviest first (walk_order_chunks)
ChunkOrder launch_walk_order_chunks(hipStream_t s, const uint32_t* off, int n_tgt, const int* info, unsigned n_groups, int* order, int mode) {
  const int ng = (int)n_groups;
  int cg = (ng + kWalkOrderChunks - 1) / kWalkOrderChunks;
  if (cg < 64) cg = 64;
  const int nc = (ng + cg - 1) / cg;
  int n_light = 8192 / (cg * 4);  // chunks of one residency round (256 CUs x 32 waves)
  if (n_light > nc / 2) n_light = nc / 2;
  walk_order_chunks<<<dim3(1), dim3(1024), 0, s>>>(off, n_tgt, info, cg, nc, order, mode, n_light);
  return ChunkOrder{order, cg, (unsigned)(nc * cg)};  // (whole chunks: the groups past the last real one find no targets and leave)
}

// development: per-wave time and step counts (walk_tile_fast<T, 0, true>; tools/walk_wave_log.py reads the file)
unsigned long long* wave_log_alloc(hipStream_t s, unsigned n_groups) {
  unsigned long long* wave_log = nullptr;
  if (hipMalloc((void**)&wave_log, (size_t)n_groups * 4 * 4 * sizeof(unsigned long long)) != hipSuccess) return nullptr;
  (void)hipMemsetAsync(wave_log, 0, (size_t)n_groups * 4 * 4 * sizeof(unsigned long long), s);
  return wave_log;
}
void wave_log_dump(hipStream_t s, unsigned long long* wave_log, unsigned n_groups) {
  const size_t nw = (size_t)n_groups * 4;
  std::vector<unsigned long long> h(nw * 4);
  (void)hipMemcpyAsync(h.data(), wave_log, nw * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(wave_log);
  const char* path = lab_str("NBODY_WALK_WAVE_LOG_FILE");
  FILE* f = fopen(path ? path : "/tmp/nbody_wave_log.bin", "wb");
  if (f) {
    fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
    fclose(f);
  }
}

}  // namespace nbody
#endif  // NBODY_LAB
