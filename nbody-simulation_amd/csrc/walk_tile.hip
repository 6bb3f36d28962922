// ---- the walk in ONE pass, terms through LDS (walk_tile) --------------------------------------------------------------
// Same idea as the three passes (walk_lab.hip) - a leaf's terms are evaluated lane = particle, so a leaf step costs what its
// takers cost - but the terms never leave the CU: up to TT acting targets of the wave are evaluated against the leaf
// (one round each, a row of the wave's LDS tile), then every one of those targets' own lanes adds its row in slice
// order (lane = target again: TT independent chains at once).  No term array (8 B per pair written and read back), no
// sum pass, no capacity to outgrow.  Waves are still cut by work; the estimate is the scan of the term counts the
// targets' particles (by id: the build permutes the rows) had in the PREVIOUS walk or, when there is none, of a
// counting traversal.  A bad estimate costs balance, never correctness: each target's additions are the fused
// walk's, in its order.  f32 and f64 (rows of 16-byte terms: half as many waves stay resident).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "walk_arms.h"
#include "walk_device.h"

namespace nbody {

namespace {

template <class T, bool FAST, int TT, bool SREC = false>
__global__ __launch_bounds__(256) void walk_tile(const WalkArgs<T> a, const uint32_t* __restrict__ off, const int* __restrict__ info,
                                                 const uint32_t* __restrict__ tgt_ids, uint32_t* __restrict__ hist,
                                                 unsigned long long* __restrict__ total_out) {
  using T2 = typename Vec2Of<T>::type;
  using T4 = typename Vec4Of<T>::type;
  constexpr int kStride = 65;  // terms per row + 1: rows of different targets start in different banks
  __shared__ T2 tile_all[4][TT * kStride];
  const int lane = threadIdx.x & 63;
  T2* __restrict__ tile = tile_all[threadIdx.x >> 6];
  const int wave = __builtin_amdgcn_readfirstlane((int)(group_of_block(a, blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)));
  if (info[1] != 0) return;  // the estimate's scan wrapped: the caller takes the fused walk
  if (wave > info[5]) return;  // past the last wave that can hold a target (most of the grid on a small scene): no searches
  // first t with g(t) >= wave, g(t) = off[t] / budget + t / 64 (see walk_pass), then the first with g(t) > wave: all on the
  // scalar side (`off` through the constant address space; the budget is a power of two, tile_total)
  const uint32_t qmul = 0xFFFFFFFFu / (uint32_t)__builtin_amdgcn_readfirstlane(info[3]);  // (budget >= 64)
  const int n_tgt = (int)a.n_tgt;  // (the scan, hence the walk, is 32 bits wide)
  int t0, lo;
  wave_targets(off, n_tgt, wave, qmul, lane, t0, lo);
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
  T ax = 0, ay = 0;  // Vec2::zero(), main.rs:409
  int i = 0;
  // The particles [first, first + count), in order, for the lanes of `mask` (`act`: this lane is one of them): main.rs:351-363.
  auto leaf_rows = [&](const unsigned long long mask, const bool act, const int first, const int count) {
    {
      {
        const int takers = __builtin_popcountll(mask);
        for (int k0 = 0; k0 < count; k0 += 64) {  // 64 particles at a time
          const int mine = k0 + lane;
          const int left = count - k0;
          const int rounds8 = ((left < 64 ? left : 64) + 7) >> 3;
          T2 q = T2{0, 0};
          T m = 0;
          if (mine < count) {
            q = lpos[first + mine];
            m = lmass[first + mine];
          }
          if (takers * kTileRoundCost > (left < 64 ? left : 64) * kFusedPairCost) {
            // most of the wave wants this leaf: lane = target, the particles one after the other (the fused walk's
            // arm; the same additions in the same order, so the two arms mix freely)
            const int mc = left < 64 ? left : 64;
            for (int j = 0; j < mc; ++j) {
              const T qx = lane_t(q.x, j), qy = lane_t(q.y, j), qm = lane_t(m, j);
              if (act) {
                const T2 term = term_of<FAST>(p.x, p.y, qx, qy, qm, clamp);
                ax = ax + term.x;
                ay = ay + term.y;
              }
            }
            continue;
          }
          unsigned long long todo = mask;
          const bool valid = mine < count;
          // the acting targets take the rows in lane order, TT per batch: a target's row is its rank among the acting lanes
          const int rank = act ? (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u)) : -1;
          int batch0 = 0;
          while (todo) {
            int slot = 0;
            while (todo && slot < TT) {  // lane = particle: one acting target per round, its terms into row `slot`
              if constexpr (!FAST && TT >= 2) {
                if (slot + 2 <= TT && (todo & (todo - 1)) != 0) {  // two acting targets are there: their rounds as one basic block
                  const int ta = __builtin_ctzll(todo);
                  todo &= todo - 1;
                  const int tb = __builtin_ctzll(todo);
                  todo &= todo - 1;
                  const T2 ra = pair_term_sel(valid, lane_t(p.x, ta), lane_t(p.y, ta), q.x, q.y, m, clamp);
                  const T2 rb = pair_term_sel(valid, lane_t(p.x, tb), lane_t(p.y, tb), q.x, q.y, m, clamp);
                  tile[slot * kStride + lane] = ra;
                  tile[(slot + 1) * kStride + lane] = rb;
                  slot += 2;
                  continue;
                }
              }
              const int tl = __builtin_ctzll(todo);
              todo &= todo - 1;
              const T tx = lane_t(p.x, tl), ty = lane_t(p.y, tl);
              if constexpr (FAST) {
                const T2 term = term_of<FAST>(tx, ty, q.x, q.y, m, clamp);
                tile[slot * kStride + lane] = valid ? term : neg_zero2<T>();  // past the leaf: the identity of addition
              } else {
                tile[slot * kStride + lane] = pair_term_if(valid, tx, ty, q.x, q.y, m, clamp);
              }
              ++slot;
            }
            const int myslot = (rank >= batch0 && rank < batch0 + slot) ? rank - batch0 : -1;
            batch0 += slot;
            wave_lds_handoff();
            if (myslot >= 0) {  // lane = target: its row, in slice order
              const T2* __restrict__ r = tile + myslot * kStride;
              if constexpr (sizeof(T) == 4) {
                // eight terms at a time, the next eight on their way from LDS while these are added (two register sets
                // taken in turn; left to itself the compiler reads a batch, waits, adds, and reads the next)
#define NB_ROW_LOAD(dst, blk) _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) dst[j_] = r[(blk) * 8 + j_];
#define NB_ROW_ADD(src) _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) { ax = ax + src[j_].x; ay = ay + src[j_].y; } \
  __builtin_amdgcn_sched_group_barrier(0x100, 8, 0); __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
                T2 va[8], vb[8];
                NB_ROW_LOAD(va, 0)
                int j0 = 0;
                for (; j0 + 3 <= rounds8; j0 += 2) {  // va holds block j0 here
                  NB_ROW_LOAD(vb, j0 + 1)
                  NB_ROW_ADD(va)
                  NB_ROW_LOAD(va, j0 + 2)
                  NB_ROW_ADD(vb)
                }
                if (j0 + 2 <= rounds8) {
                  NB_ROW_LOAD(vb, j0 + 1)
                  NB_ROW_ADD(va)
                  NB_ROW_ADD(vb)
                } else {
                  NB_ROW_ADD(va)
                }
#undef NB_ROW_LOAD
#undef NB_ROW_ADD
              } else {
                for (int j0 = 0; j0 < rounds8; ++j0) {
                  T2 v[8];
#pragma unroll
                  for (int j = 0; j < 8; ++j) v[j] = r[j0 * 8 + j];
#pragma unroll
                  for (int j = 0; j < 8; ++j) {
                    ax = ax + v[j].x;
                    ay = ay + v[j].y;
                  }
                }
              }
            }
            wave_lds_handoff();
          }
        }
      }
    }
  };
  while (i < n_nodes) {  // i is wave-uniform
    const NodeRec<T> rec = SREC ? scalar_node_rec<T>(a.link, a.geom0, a.geom1, i) : NodeRec<T>{lk[i], g0[i], g1[i]};
    const int4 l = rec.l;
    const T4 b = rec.b;
    const T4 c = rec.c;
#ifndef NB_TILE_LATE_GEOM
    asm volatile("" : : "s"(b.x), "s"(c.w));  // the three records together: one latency per step (the compiler sinks the two
                                              // it needs in the node arm only into that arm, behind the first one's wait)
#endif
    const bool act = resume <= i;
    int next;
    if (l.w) {  // Leaf arm
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(act);
      if (mask) leaf_rows(mask, act, l.y, l.z);
      if (act) {
        n_terms += (uint32_t)l.z;
        resume = l.x;
      }
      next = l.x;
    } else {
      // The node test as straight-line code: compares and-ed as masks, selects instead of nested exec regions (what `if (act) { if
      // (...) {...} else {...} }` compiles to: four s_and_saveexec / s_or exec pairs, their copies and branches — about half of the
      // ≈ 100 instructions of a node step, which is what a wave that runs alone pays for: it issues one instruction per ≈ 8-15 cycles).
      const bool contains = (p.y > b.y) & (p.x > b.x) & (p.x < b.z) & (p.y < b.w);  // bvh_tree.rs:15-20 (all strict)
      const T ddx = p.x - c.x, ddy = p.y - c.y;                                   // dist2(p, cog), main.rs:228-232
      const T d2 = ddx * ddx + ddy * ddy;
      const bool accept = act & !contains & (c.w < d2 * theta * theta);              // :370-372
      const bool descend = act & !accept;                                            // :381-382
      if (__builtin_amdgcn_ballot_w64(accept) != 0) {  // (wave-uniform: the as-written term is two IEEE divisions)
        const T2 term = term_of<FAST>(p.x, p.y, c.x, c.y, c.z, clamp);               // :374-379
        const T nax = ax + term.x, nay = ay + term.y;
        ax = accept ? nax : ax;
        ay = accept ? nay : ay;
      }
      n_terms += accept ? 1u : 0u;
      resume = accept ? l.x : (descend ? i + 1 : resume);
      const unsigned long long dmask = __builtin_amdgcn_ballot_w64(descend);
      if (l.x - i == 3) {
        // A subtree of three nodes: both children are leaves and a lane that descends takes both, whole (main.rs:381-382:
        // children[0] then children[1]) — their slices, one after the other, ARE this node's own range [first, first +
        // count) (the partition keeps a node's particles together, left child first; the record of an inner node carries
        // its range too).  So the two leaf steps happen here: the same pairs for the same lanes in the same order, two
        // records and one round trip to the particles fewer per pair of leaves.
        if (dmask) leaf_rows(dmask, descend, l.y, l.z);
        if (descend) {
          n_terms += (uint32_t)l.z;
          resume = l.x;
        }
        next = l.x;
      } else {
        next = dmask != 0 ? i + 1 : l.x;
      }
    }
    i = __builtin_amdgcn_readfirstlane(next);
  }
  if (live) {
    reinterpret_cast<T2*>(a.acc)[row] = T2{ax, ay};
    if (hist) hist[tgt_ids[t]] = n_terms;  // by particle id: the rows are permuted by every build
  }
  unsigned long long sum = live ? n_terms : 0ull;  // what this walk cost, for the next estimate's scale
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
  if (lane == 0) atomicAdd(total_out, sum);
}

// The product ships rows 8 with scalar node records; every other instantiation is the laboratory's.
template <class T, bool FAST, int TT> hipError_t launch_rows_of(const TileLaunch& k, const WalkArgs<T>& a, const bool srec) {
  if (srec) {
    walk_tile<T, FAST, TT, true><<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
    return hipGetLastError();
  }
  if constexpr (kLabBuild) {
    walk_tile<T, FAST, TT, false><<<k.grid, dim3(256), 0, k.s>>>(a, k.off, k.info, k.tgt_ids, k.hist, k.total_out);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}
template <class T, bool FAST> hipError_t launch_rows(const TileLaunch& k, const WalkArgs<T>& a, const TileRoute& rt) {
  if (rt.rows == 8) return launch_rows_of<T, FAST, 8>(k, a, rt.srec != 0);
  if constexpr (kLabBuild) {
    if (rt.rows == 16) return launch_rows_of<T, FAST, 16>(k, a, rt.srec != 0);
    if (rt.rows == 4) return launch_rows_of<T, FAST, 4>(k, a, rt.srec != 0);
  }
  return hipErrorInvalidValue;
}

}  // namespace

template <class T> hipError_t launch_walk_tile_rows(const TileLaunch& k, const WalkArgs<T>& a, const TileRoute& rt) {
  if (arm_is(rt, "exact")) return launch_rows<T, false>(k, a, rt);
  if constexpr (kLabBuild || sizeof(T) == 8) {  // FAST through the rows: f64 (the f32 product walks through registers)
    if (arm_is(rt, "fast-rows")) return launch_rows<T, true>(k, a, rt);
  }
  return hipErrorInvalidValue;
}

template hipError_t launch_walk_tile_rows<float>(const TileLaunch&, const WalkArgs<float>&, const TileRoute&);
template hipError_t launch_walk_tile_rows<double>(const TileLaunch&, const WalkArgs<double>&, const TileRoute&);

}  // namespace nbody
