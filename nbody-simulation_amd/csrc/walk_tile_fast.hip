// ---- the one-pass walk under the TOLERANCE contract (nbody_arith FAST) --------------------------------------------------
// north_star asks bit parity of the tree INDEXING and a tolerance on the forces.  walk_tile (walk_tile.hip) pays for bit parity of the
// sums as well: a row of LDS per target, a fenced hand-off, 64 dependent adds per target and leaf, two IEEE divisions per
// pair (76 VALU instructions per (target, leaf) round).  walk_tile_fast keeps the traversal — same node tests, same
// interaction lists, so nbody_tree_walk_stats and the history are the exact walk's — and spends the freedom:
//   * a pair costs one v_rcp (pair_term_fast: the direct kernel's arithmetic and tolerance) and lands in an FMA;
//   * lane = particle rounds keep their 64 terms in registers; eight targets' rows are summed TOGETHER by a transposed
//     reduction: v_permlane32_swap + add (8 -> 4 values, each half-wave another target), v_permlane16_swap + add (4 -> 2,
//     each row of 16 lanes another target), a DPP rotate by 8 lanes + add under a bank mask (2 -> 1), three DPP adds inside
//     8 lanes: 36 instructions per coordinate pair for eight targets, no LDS, no fence, no chain;  each target's lane
//     fetches its total with one ds_bpermute per coordinate;
//   * where most of the wave wants the leaf the particles are broadcast instead (lane = target), as before.
// Any order of additions is inside the tolerance (tests/_tol.py: 2e-5 of sum |term|; a tree of 64 + one add per leaf is
// a better-conditioned sum than the reference's sequential chain).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "walk_arms.h"
#include "walk_device.h"

namespace nbody {

namespace {

template <class T, int REC, bool LOG>  // REC: how the node records are fetched (0 plain loads: the compiler picks scalar loads; 1 vector loads); LOG: per-wave log (development)
__global__ __launch_bounds__(256) void walk_tile_fast(const WalkArgs<T> a, const uint32_t* __restrict__ off, const int* __restrict__ info,
                                                      const uint32_t* __restrict__ tgt_ids, uint32_t* __restrict__ hist,
                                                      unsigned long long* __restrict__ total_out) {
  using T2 = typename Vec2Of<T>::type;
  using T4 = typename Vec4Of<T>::type;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(group_of_block(a, blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)));
  if (info[1] != 0) return;  // the estimate's scan wrapped: the caller walks again without one
  if (wave > info[5]) return;  // past the last wave that can hold a target (most of the grid on a small scene): no searches
  const long long log_t0 = LOG ? wall_clock64() : 0;
  // Which targets are this wave's: those with g(t) = off[t] / budget + t / 64 == wave (see walk_pass), by two binary searches.
  // Everything in them is wave-uniform, and kept on the scalar side on purpose: `off` is read through the constant address
  // space (s_load: it was written by kernels before this one) and the budget is a power of two (tile_total), so the
  // quotient is a shift — forty dependent steps that cost a wave 125 us as vector loads and a 32-bit division each, on
  // SIMDs whose vector pipes the other waves keep busy (profiles/r03_walk_wave_log.txt).
  const uint32_t qmul = 0xFFFFFFFFu / (uint32_t)__builtin_amdgcn_readfirstlane(info[3]);  // (budget >= 64)
  const int n_tgt = (int)a.n_tgt;  // (the scan, hence the walk, is 32 bits wide)
  int t0, lo;
  wave_targets(off, n_tgt, wave, qmul, lane, t0, lo);
  const long long log_t1 = LOG ? wall_clock64() : 0;  // the search is over (its ballots waited for its loads)
  if (lo == t0) return;
  const int64_t t = (int64_t)t0 + lane;
  const bool live = t < lo;
  const int64_t row = live ? (a.tgt_index ? (int64_t)a.tgt_index[t] : t) : 0;
  const T2 p = live ? reinterpret_cast<const T2*>(a.tgt_pos)[row] : T2{0, 0};
  const T4* __restrict__ g0 = reinterpret_cast<const T4*>(a.geom0);
  const T4* __restrict__ g1 = reinterpret_cast<const T4*>(a.geom1);
  const int4* __restrict__ lk = reinterpret_cast<const int4*>(a.link);
  const T2* __restrict__ lpos = reinterpret_cast<const T2*>(a.leaf_pos);
  const T* __restrict__ lmass = a.leaf_mass;
  const T theta = a.theta, clamp = a.clamp;
  const int n_nodes = a.n_nodes_dev ? __builtin_amdgcn_readfirstlane(*a.n_nodes_dev) : a.n_nodes;
  int resume = live ? 0 : n_nodes;
  uint32_t n_terms = 0;
  // Two-level summation, as in the direct kernel: the terms go to a block sum (bx, by) that joins the running total after every fourth
  // leaf step.  A target's list can be a large part of all particles (small theta on the BVH's needle boxes; all-negative
  // coordinates, whose boxes stretch to the origin: bvh_tree.rs:42) and a plain f32 chain of N additions drifts by ~sqrt(N)
  // half-ulps of the sum of magnitudes: 2.2e-5 ... 4.9e-5 of it on lists of 2 x 10^4 ... 10^5 terms (found by the extended fuzz;
  // the contract is 2e-5).
  T ax = 0, ay = 0, bx = 0, by = 0;
  int leaf_steps = 0;
  auto flush_if_due = [&]() {
    if (++leaf_steps == 4) {
      ax = ax + bx;
      ay = ay + by;
      bx = by = 0;
      leaf_steps = 0;
    }
  };
  int i = 0;
  unsigned log_nodes = 0, log_leaves = 0, log_rounds = 0;
  // A node's three records (link, box, centre of gravity | mass | s^2), fetched together: one latency per step.  REC = 1
  // fetches them by VECTOR loads of one address (the offset passes through a register the compiler cannot see through, or
  // it would pick scalar loads): the records then sit in VGPRs, where the node test's operands cost half of what SGPR
  // operands cost (measured cost model).  Measured equal within 2 % (profiles/r03_walk_fast_variants.txt);
  // fetching one node AHEAD into a second register set made both scenes 12-15 % slower (the compiler copies the set at the
  // loop's back edge behind a full wait).
  struct Rec { int4 l; T4 b; T4 c; };
  const int last = n_nodes - 1;
  unsigned lane_zero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(lane_zero));
  auto fetch = [&](int k) -> Rec {
    k = k < last ? k : last;
    if constexpr (REC == 3) {  // scalar loads through the constant address space (scalar_node_rec)
      const NodeRec<T> r = scalar_node_rec<T>(a.link, a.geom0, a.geom1, k);
      asm volatile("" : : "s"(r.b.x), "s"(r.c.w));  // the three records together, before anything branches on the first
      return Rec{r.l, r.b, r.c};
    }
    if constexpr (REC == 0) {
      const Rec r{lk[k], g0[k], g1[k]};
      asm volatile("" : : "s"(r.b.x), "s"(r.c.w));  // (as in walk_tile: without it the compiler sinks the box and the centre of gravity
      return r;                                     // into the node arm, behind the link's wait: two round trips per node step)
    }
    const unsigned o16 = (unsigned)k * 16u + lane_zero;
    const unsigned ot = (unsigned)k * (unsigned)sizeof(T4) + lane_zero;
    return Rec{*reinterpret_cast<const int4*>(reinterpret_cast<const char*>(lk) + o16), *reinterpret_cast<const T4*>(reinterpret_cast<const char*>(g0) + ot),
               *reinterpret_cast<const T4*>(reinterpret_cast<const char*>(g1) + ot)};
  };
  // The particles [first, first + count) for the lanes of `mask` (`taker`: this lane is one of them), main.rs:351-363;
  // any order of additions (tolerance contract).
  auto rounds = [&](const unsigned long long mask, const bool taker, const int first, const int count) {
    {
      {
        const bool act = taker;
        const int takers = __builtin_popcountll(mask);
        if constexpr (LOG) { ++log_leaves; log_rounds += (unsigned)takers; }
        const int rank = act ? (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u)) : -1;
        for (int k0 = 0; k0 < count; k0 += 64) {  // 64 particles at a time
          const int mine = k0 + lane;
          const int left = count - k0;
          const int mc = left < 64 ? left : 64;
          T2 q = T2{0, 0};
          T m = 0;  // a lane past the end: force 0, its terms are exact zeros
          if (mine < count) {
            q = lpos[first + mine];
            m = lmass[first + mine];
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
          // one acting target's terms against the 64 particles, lane = particle
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
              for (int sl = 0; sl < 5; ++sl) NB_FAST_ROUND(X[sl], Y[sl])  // (five are there: one basic block, so the scheduler
#pragma unroll                                                            // interleaves their chains — what a wave that runs alone lives on)
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
              for (int sl = 0; sl < 3; ++sl) NB_FAST_ROUND(V[2 * sl], V[2 * sl + 1])  // (three are there)
              V[6] = 0;
              V[7] = 0;
              if (todo) NB_FAST_ROUND(V[6], V[7])
              const T r = reduce8(V);
              const int src = 16 * (k & 1) + 8 * ((k >> 1) & 1);  // slot_lane8(2k); y sits 32 lanes on (slot_lane8(2k + 1))
              gx = lane_fetch(r, src);
              gy = lane_fetch(r, src + 32);
              took = 4;
            } else if (left_t == 2) {  // two targets: four values
              T V[4];
              NB_FAST_ROUND(V[0], V[1])
              NB_FAST_ROUND(V[2], V[3])
              const T r = reduce4(V);  // x0 row 0, y0 row 2, x1 row 1, y1 row 3
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
    }
  };
  auto step = [&](const Rec& rec, const int i) -> int {
    const int4 l = rec.l;
    const T4 b = rec.b;
    const T4 c = rec.c;
    const bool act = resume <= i;
    int next;
    if (l.w) {  // Leaf arm
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(act);
      if (mask) {
        rounds(mask, act, l.y, l.z);
        flush_if_due();
      }
      if (act) {
        n_terms += (uint32_t)l.z;
        resume = l.x;
      }
      next = l.x;
    } else {
      if constexpr (LOG) ++log_nodes;
      // straight-line: masks and selects instead of nested exec regions (see walk_tile); the term is computed for every lane and
      // kept by the lanes that accept (a select on the RESULT: an empty node's centre of gravity is NaN, and NaN x 0 is not 0)
      const bool contains = (p.y > b.y) & (p.x > b.x) & (p.x < b.z) & (p.y < b.w);  // bvh_tree.rs:15-20 (all strict)
      const T ddx = p.x - c.x, ddy = p.y - c.y;                                   // dist2(p, cog), main.rs:228-232
      const T d2 = ddx * ddx + ddy * ddy;
      const bool accept = act & !contains & (c.w < d2 * theta * theta);              // :370-372 (the test is the exact walk's, bit for bit)
      const bool descend = act & !accept;                                            // :381-382
      const T dx = c.x - p.x, dy = c.y - p.y;                                        // :374-379
      const T sc = fast_scale(dx, dy, c.z, clamp);
      const T nbx = fma_t(dx, sc, bx), nby = fma_t(dy, sc, by);
      bx = accept ? nbx : bx;
      by = accept ? nby : by;
      n_terms += accept ? 1u : 0u;
      resume = accept ? l.x : (descend ? i + 1 : resume);
      const unsigned long long dmask = __builtin_amdgcn_ballot_w64(descend);
      if (l.x - i == 3) {
        // A subtree of three nodes: both children are leaves, and a lane that descends here takes both, whole — their
        // particles are this node's own range [first, first + count) (a node's record carries its range too).  So the two
        // leaf steps happen HERE: two records and one round trip for the particles fewer per pair of leaves, which is most of
        // what a wave waits for (the records of three leaves in four are never fetched).  Same pairs, same lanes.
        if (dmask) {
          rounds(dmask, descend, l.y, l.z);
          flush_if_due();
        }
        if (descend) {
          n_terms += (uint32_t)l.z;
          resume = l.x;
        }
        next = l.x;
      } else {
        next = dmask != 0 ? i + 1 : l.x;
      }
    }
    return __builtin_amdgcn_readfirstlane(next);
  };
  long long log_t2 = 0;
  while (i < n_nodes) {
    const Rec r = fetch(i);
    if (LOG && i == 0) {
      asm volatile("" : : "s"(r.l.x), "v"(p.x));  // the root's record and the targets have arrived
      log_t2 = wall_clock64();
    }
    i = step(r, i);
  }
  const long long log_t3 = LOG ? wall_clock64() : 0;  // the walk is over: what follows is the wave's epilogue
  ax = ax + bx;
  ay = ay + by;
  if (live) {
    reinterpret_cast<T2*>(a.acc)[row] = T2{ax, ay};
    if (hist) hist[tgt_ids[t]] = n_terms;  // by particle id: the rows are permuted by every build
  }
  unsigned long long sum = live ? n_terms : 0ull;  // what this walk cost, for the next estimate's scale
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
  if (lane == 0) atomicAdd(total_out, sum);
  if (LOG && lane == 0) {
    unsigned long long* o = a.wave_log + 4 * wave;
    o[0] = (((unsigned long long)log_t0 & 0xFFFFFFFFFFull) << 24) | ((unsigned long long)(wall_clock64() - log_t0) & 0xFFFFFFull);  // start (absolute, 40 bits) | duration
    o[1] = (unsigned long long)log_nodes | ((unsigned long long)((log_t1 - log_t0) & 0xFFFF) << 32) | ((unsigned long long)((log_t2 - log_t0) & 0xFFFF) << 48);  // + ticks to the end of the search | to the first record
    o[2] = (unsigned long long)log_leaves | ((unsigned long long)((wall_clock64() - log_t3) & 0xFFFF) << 32);  // + ticks of the epilogue
    o[3] = ((unsigned long long)(unsigned)(lo - t0) << 32) | log_rounds;
  }
}

}  // namespace

// The product ships the f32 walk with node records by scalar loads (REC 3); the other record modes, the per-wave log and the f64
// register walk are the laboratory's.
template <class T> hipError_t launch_walk_tile_fast(const TileLaunch& k, const WalkArgs<T>& a, const TileRoute& rt) {
  if constexpr (kLabBuild || sizeof(T) == 4) {
    const bool log = arm_is(rt, "fast-registers-log");
    if (!log && !arm_is(rt, "fast-registers")) return hipErrorInvalidValue;
    if (!log && rt.rec_mode == 3) {
      walk_tile_fast<T, 3, false><<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
      return hipGetLastError();
    }
    if constexpr (kLabBuild) {
      if (log && rt.rec_mode == 0 && a.wave_log) walk_tile_fast<T, 0, true><<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
      else if (!log && rt.rec_mode == 1) walk_tile_fast<T, 1, false><<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
      else if (!log && rt.rec_mode == 0) walk_tile_fast<T, 0, false><<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
      else return hipErrorInvalidValue;
      return hipGetLastError();
    }
  }
  return hipErrorInvalidValue;
}

template hipError_t launch_walk_tile_fast<float>(const TileLaunch&, const WalkArgs<float>&, const TileRoute&);
template hipError_t launch_walk_tile_fast<double>(const TileLaunch&, const WalkArgs<double>&, const TileRoute&);

}  // namespace nbody
