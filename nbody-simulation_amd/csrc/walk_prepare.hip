// The one-pass walk's preparation (walk_tile.hip, walk_tile_fast.hip walk afterwards): an estimate of every target's terms — a
// counting traversal, or the counts of the previous walk — its exclusive scan and overflow check, the waves' budget, and what a
// step enqueued ahead of the host lets ride along (TileTail, walk_split.h).  The one unit of the walk that needs the library scan.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>

#include "bvh_build.h"
#include "env.h"
#include "walk_arms.h"
#include "walk_device.h"
#include "walk_split.h"

namespace nbody {

namespace {

// Waves the one-pass walk aims at; a wave's budget is total terms / (this - n / 64), any integer (tile_budget).  Round 4, measured
// (profiles/r04_walk_wave_target.txt): the walk is its longest waves' chains, and they all start at once only while EVERY wave is
// resident — 256 CUs x 32 slots = 8 192.  Round 3 aimed at 16 384 ("twice what the chip holds") with power-of-two budgets: 9 700 waves
// on the bench's reference-scene leg, a second residency round (exact 0.636 ms, FAST 0.338).  Kept inside one round the same walk takes
// 0.48-0.49 / 0.29-0.30 ms; Plummer 262 144: 0.76 -> 0.61-0.63, 400 000: 1.32 -> 1.15.  Where the head count alone exceeds the
// chip (n / 64 > 8 192) every extra wave repeats a traversal for nothing: 1 024 more than the head count is the measured optimum at
// 400 000, 655 360 and 1 048 576 bodies.
__host__ __device__ inline int64_t tile_waves_target(int64_t n_tgt) {
  const int64_t w = n_tgt / 64 + 1024;
  return w > 6656 ? w : 6656;
}

// The counting traversal for either precision: node tests only (walk_pass<false> is its f32 twin).
template <class T>
__global__ __launch_bounds__(256) void walk_count(const WalkArgs<T> a, uint32_t* __restrict__ cnt) {
  using T2 = typename Vec2Of<T>::type;
  using T4 = typename Vec4Of<T>::type;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < a.n_tgt;
  const int64_t row = live ? (a.tgt_index ? (int64_t)a.tgt_index[t] : t) : 0;
  const T2 p = live ? reinterpret_cast<const T2*>(a.tgt_pos)[row] : T2{0, 0};
  const T4* __restrict__ g0 = reinterpret_cast<const T4*>(a.geom0);
  const T4* __restrict__ g1 = reinterpret_cast<const T4*>(a.geom1);
  const int4* __restrict__ lk = reinterpret_cast<const int4*>(a.link);
  const T theta = a.theta;
  const int n_nodes = a.n_nodes;
  int resume = live ? 0 : n_nodes;
  uint32_t n_terms = 0;
  int i = 0;
  while (i < n_nodes) {
    const int4 l = lk[i];
    const T4 b = g0[i];
    const T4 c = g1[i];
    const bool act = resume <= i;
    int next;
    if (l.w) {
      if (act) {
        n_terms += (uint32_t)l.z;
        resume = l.x;
      }
      next = l.x;
    } else {
      bool descend = false;
      if (act) {
        const bool contains = p.y > b.y && p.x > b.x && p.x < b.z && p.y < b.w;
        const T ddx = p.x - c.x, ddy = p.y - c.y;
        const T d2 = ddx * ddx + ddy * ddy;
        if (!contains && c.w < d2 * theta * theta) {
          ++n_terms;
          resume = l.x;
        } else {
          descend = true;
          resume = i + 1;
        }
      }
      next = __builtin_amdgcn_ballot_w64(descend) != 0 ? i + 1 : l.x;
    }
    i = __builtin_amdgcn_readfirstlane(next);
  }
  if (live) cnt[t] = n_terms;
}

__global__ __launch_bounds__(256) void walk_check_wrap(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, int64_t n,
                                                       int* __restrict__ info) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i + 1 < n && (unsigned long long)off[i] + cnt[i] != (unsigned long long)off[i + 1]) {  // the 32-bit scan wrapped
    info[1] = 1;
    info[2] = 1;
  }
}

struct EstimateOf {  // target t's terms in the last walk, scaled
  const uint32_t* hist;
  const uint32_t* ids;
  int shift;
  __host__ __device__ __forceinline__ uint32_t operator()(int t) const { return hist ? hist[ids[t]] >> shift : 0u; }
};
// the scan of a history estimate must not wrap either: the shift is sized from the last walk's total, but a target set
// that is not the last one (a shard's slice moves with the tree order) may hold counts of older walks
__global__ __launch_bounds__(256) void walk_check_wrap_est(EstimateOf est, const uint32_t* __restrict__ off, int64_t n, int* __restrict__ info) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i + 1 < n && (unsigned long long)off[i] + est((int)i) != (unsigned long long)off[i + 1]) {
    info[1] = 1;
    info[2] = 1;
  }
  if (i + 1 == n && (unsigned long long)off[i] + est((int)i) > 0x7fffffffull) info[1] = 1;  // the budget arithmetic is 31 bits wide
}
// budget of walk_tile's waves from the estimate's total (see walk_total)
// A wave's budget in (scaled) terms: total / extra_waves rounded up — g(t) = off[t] / budget + t / 64 then ends within extra_waves of the
// head count — never below kTileBudget (scaled like the estimate) or 64.
__device__ __forceinline__ uint32_t tile_budget(unsigned long long total, int64_t extra_waves, int shift) {
  const unsigned long long want = (total + (unsigned long long)extra_waves - 1) / (unsigned long long)extra_waves;
  unsigned long long budget = kTileBudget >> shift;
  if (budget < 64) budget = 64;
  if (budget < want) budget = want;
  if (budget > (1ull << 30)) budget = 1ull << 30;
  return (uint32_t)budget;
}
__device__ __forceinline__ void tile_total(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, int64_t n,
                                           const uint32_t* __restrict__ tgt_ids, const uint32_t* __restrict__ hist, int shift,
                                           int64_t extra_waves, int64_t grid_waves, int* __restrict__ info) {
  const uint32_t last = n > 0 ? (cnt ? cnt[n - 1] : (hist ? hist[tgt_ids[n - 1]] >> shift : 0u)) : 0u;
  const unsigned long long total = n > 0 ? (unsigned long long)off[n - 1] + last : 0ull;
  info[0] = (int)(total > 0x7fffffffull ? 0x7fffffffull : total);
  // g(t) = off[t] / budget + t / 64 ends near total / budget + n / 64: `extra_waves` more than the head count alone
  // (ceiling: with the floor, total / budget could reach extra_waves + extra_waves / want, past the grid)
  const uint32_t budget = tile_budget(total, extra_waves, shift);
  info[3] = (int)budget;
  info[5] = (int)(total / budget + (unsigned long long)((n > 0 ? n - 1 : 0) / 64));  // the last wave that can hold a target (g of the last one)
  // belt and braces: a wave index the grid does not hold would leave its targets unwalked — flag it like a wrapped scan,
  // the host then repeats the walk without an estimate (64 targets per wave, which always fits)
  if (total / budget + (unsigned long long)(n / 64) + 1 >= (unsigned long long)grid_waves) info[1] = 1;
  info[6] = info[7] = 0;  // this walk's total terms (unsigned long long), accumulated by walk_tile
}
__global__ void walk_tile_total(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, int64_t n, const uint32_t* __restrict__ tgt_ids,
                                const uint32_t* __restrict__ hist, int shift, int64_t extra_waves, int64_t grid_waves,
                                int* __restrict__ info) {
  tile_total(cnt, off, n, tgt_ids, hist, shift, extra_waves, grid_waves, info);
}
// The TileTail duties (walk_split.h), by the one work-group that knows the estimate's total: the walk's budget and flags
// (info[0..7] final), the verdict on the build, the record packed for the host, the build's counters cleared.
__device__ __forceinline__ void tile_tail_duties(unsigned long long total, int wrapped, int wrapped2, int shift, int64_t n, int64_t extra_waves,
                                                 int64_t grid_waves, int groups, int* __restrict__ info, const TileTail& tail, int tid) {
  const int my_flag = tail.pack && tid < tail.flag_words ? tail.flags[tid] : 0;  // (on its way while thread 0 works)
  if (tid == 0) {
    int out[8] = {0, wrapped, wrapped2, 0, 0, 0, 0, 0};
    out[0] = (int)(total > 0x7fffffffull ? 0x7fffffffull : total);
    // walk_tile_total's arithmetic (a total clipped to 2^31 - 1 has raised the flag already)
    const uint32_t budget = tile_budget(total, extra_waves, shift);
    out[3] = (int)budget;
    out[5] = (int)(total / budget + (unsigned long long)((n > 0 ? n - 1 : 0) / 64));  // the last wave that can hold a target
    if (total / budget + (unsigned long long)(n / 64) + 1 >= (unsigned long long)grid_waves) out[1] = 1;
    out[4] = groups;
#pragma unroll
    for (int k = 0; k < 8; ++k) info[k] = out[k];
    int v0 = 0, v1 = 0;
    if (tail.verdict) {
      const int m = tail.flags[kBvhNodes];
      const bool ok = tail.flags[kBvhFallback] == 0 && tail.flags[kBvhBadIndex] == 0 && m > 0 && m <= tail.node_cap &&
                      tail.flags[kBvhNodeCount] <= tail.node_cap &&
                      (tail.level_end <= 0 || tail.bigcount[tail.level_end] == 0);
      v0 = ok ? m : 0;
      v1 = ok ? 1 : 0;
      tail.verdict[0] = v0;
      tail.verdict[1] = v1;
    }
    if (tail.pack) {
      tail.pack[0] = v0;
      tail.pack[1] = v1;
#pragma unroll
      for (int k = 0; k < 8; ++k) tail.pack[2 + tail.flag_words + k] = out[k];
    }
  }
  if (tail.pack && tid < tail.flag_words) tail.pack[2 + tid] = my_flag;
  __syncthreads();  // the flags are in registers or packed: the next build's counters may go
  for (int k = tid; k < tail.clear_words; k += 256) tail.clear[k] = 0;
}

// walk_check_wrap_est, and in the work-group that finishes last: walk_tile_total and the TileTail duties (walk_split.h).
// info[4] counts the finished groups, info[5] takes the estimate's total from the thread that meets the last target (zero
// before, like the rest of info).
__global__ __launch_bounds__(256) void walk_check_est_tail(EstimateOf est, const uint32_t* __restrict__ off, int64_t n, int64_t extra_waves,
                                                           int64_t grid_waves, int* __restrict__ info, const TileTail tail) {
  __shared__ int last_group;
  const int tid = threadIdx.x;
  // (few groups, each over many targets: every group ends with an atomic on ONE counter, ~60 ns apiece)
  // four targets per thread and round, their loads side by side (a dependent gather each: hist[ids[i]])
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + tid; i0 < n; i0 += 4 * stride) {
    uint32_t o[4], e[4], nx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = i0 + k * stride;
      o[k] = i < n ? off[i] : 0u;
      e[k] = i < n ? est((int)i) : 0u;
      nx[k] = i + 1 < n ? off[i + 1] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = i0 + k * stride;
      const unsigned long long end = (unsigned long long)o[k] + e[k];
      if (i + 1 < n && end != (unsigned long long)nx[k]) {
        info[1] = 1;
        info[2] = 1;
      }
      if (i + 1 == n) {
        if (end > 0x7fffffffull) info[1] = 1;  // the budget arithmetic is 31 bits wide
        info[5] = (int)(end > 0x7fffffffull ? 0x7fffffffull : end);
      }
    }
  }
  __threadfence();  // the flags above, before this group counts as finished
  __syncthreads();
  if (tid == 0) last_group = atomicAdd(&info[4], 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!last_group) return;
  __threadfence();
  // what the other groups left, past this compute unit's cache
  const int wrapped = __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int wrapped2 = __hip_atomic_load(&info[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long total = (unsigned long long)(unsigned)__hip_atomic_load(&info[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tile_tail_duties(total, wrapped, wrapped2, est.shift, n, extra_waves, grid_waves, (int)gridDim.x, info, tail, tid);
}

// The estimate's exclusive scan, its overflow check and the TileTail duties in ONE launch (the step enqueued ahead of the host
// spent three on them: the library scan's two kernels and walk_check_est_tail, 32 us of a 1.1 ms step).  A single-pass scan
// with decoupled look-back: a work-group takes a ticket (arrival order, so every predecessor is running or done), scans its
// 1 024 estimates, publishes its aggregate, looks back over its predecessors' states until it meets an inclusive prefix, and
// publishes its own.  States are 64-bit words {epoch : 30 | flag : 2 | value : 32} read and written whole; the epoch (the high
// half of the ticket word st[0], drawn with the ticket by one 64-bit atomicAdd; the work-group with the last ticket stores
// {epoch + 1, ticket 0}: by then every group has drawn) makes last launch's states invisible, so the host clears the area once, when it allocates it, and
// keeps no books.  Values saturate at 2^31: a total that large is the overflow the walk must not run with (the old check's
// wrapped 32-bit sums), and offsets are not needed then.  A look-back that waits absurdly long gives up with a saturated
// prefix: the walk is then skipped and the host walks the plain way — never a hang.  The work-group with the last ticket
// knows the total and does the tail's duties.
constexpr int kScanPer = 4;
constexpr int64_t kFusedScanMaxTargets = (int64_t)1 << 24;
constexpr unsigned long long kScanSat = 0x80000000ull;
constexpr unsigned long long kScanAgg = 1ull, kScanPrefix = 2ull;
__device__ __forceinline__ unsigned long long scan_word(unsigned epoch, unsigned long long flag, unsigned long long v) {
  return ((unsigned long long)epoch << 34) | (flag << 32) | (v > kScanSat ? kScanSat : v);
}
__global__ __launch_bounds__(256) void walk_scan_est_tail(EstimateOf est, uint32_t* __restrict__ off, int64_t n, unsigned long long* __restrict__ st,
                                                          int64_t extra_waves, int64_t grid_waves, int* __restrict__ info, const TileTail tail) {
  __shared__ unsigned s_b, s_epoch;
  __shared__ unsigned long long s_wave[4], s_excl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0 && blockIdx.x == 0 && tail.stamp) *tail.stamp = (unsigned long long)wall_clock64();
  if (tid == 0) {
    // ticket (low word) and epoch (high word) come out of ONE 64-bit atomic: two separate relaxed accesses to two addresses are not
    // ordered by the memory model, and a group that took an early ticket but read the epoch the last group had already advanced
    // would publish and wait under the wrong epoch
    const unsigned long long te = atomicAdd(&st[0], 1ull);
    s_b = (unsigned)te;
    s_epoch = (unsigned)(te >> 32) & 0x3FFFFFFFu;
  }
  __syncthreads();
  const unsigned b = s_b, epoch = s_epoch;
  unsigned long long* __restrict__ state = st + 2;
  const int64_t i0 = ((int64_t)b * 256 + tid) * kScanPer;
  uint32_t e[kScanPer];
  unsigned long long tsum = 0ull;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    e[k] = i0 + k < n ? est((int)(i0 + k)) : 0u;
    tsum += e[k];
  }
  unsigned long long inc = tsum;  // inclusive over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = (unsigned long long)__shfl_up((long long)inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  unsigned long long before = 0ull, block_total = 0ull;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += s_wave[w];
    block_total += s_wave[w];
  }
  if (wave == 0) {
    unsigned long long excl = 0ull;
    if (b > 0) {
      if (lane == 0) __hip_atomic_store(&state[b], scan_word(epoch, kScanAgg, block_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (long long j = (long long)b - 1;; j -= 64) {  // 64 predecessors at a time, the nearest in lane 0
        const long long idx = j - lane;
        unsigned long long v = scan_word(epoch, kScanPrefix, 0ull);  // before the first work-group: an empty prefix
        if (idx >= 0) {
          int patience = 1 << 20;
          for (;;) {  // (its owner holds an earlier ticket: it is on its way.  The states carry their own data: relaxed loads do)
            v = __hip_atomic_load(&state[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (((unsigned)(v >> 34) == epoch && ((v >> 32) & 3ull) != 0ull) || --patience <= 0) break;
            __builtin_amdgcn_s_sleep(2);
          }
          if (patience <= 0) v = scan_word(epoch, kScanPrefix, kScanSat);  // give up: saturated, the walk will not run on this scan
        }
        const unsigned long long has_prefix = __builtin_amdgcn_ballot_w64(((v >> 32) & 3ull) == kScanPrefix);
        const int stop = has_prefix ? __builtin_ctzll(has_prefix) : 63;  // lanes 0 .. stop count
        unsigned long long part = lane <= stop ? (v & 0xFFFFFFFFull) : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += (unsigned long long)__shfl_xor((long long)part, d, 64);
        excl += part;
        if (excl > kScanSat) excl = kScanSat;
        if (has_prefix) break;
      }
    }
    if (lane == 0) {
      __hip_atomic_store(&state[b], scan_word(epoch, kScanPrefix, excl + block_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_excl = excl;
    }
  }
  __syncthreads();
  const unsigned long long excl = s_excl;
  unsigned long long run = excl + before + (inc - tsum);
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    if (i0 + k < n) off[i0 + k] = (uint32_t)run;
    run += e[k];
  }
  if (b + 1 != gridDim.x) return;
  if (tid == 0)  // every group holds its ticket and, with it, the epoch: the word moves on to {epoch + 1, ticket 0} in one store
    __hip_atomic_store(&st[0], (unsigned long long)((epoch + 1u) & 0x3FFFFFFFu) << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long total = excl + block_total;
  if (total > kScanSat) total = kScanSat;
  const int wrapped = total > 0x7fffffffull ? 1 : 0;
  tile_tail_duties(total, wrapped, wrapped, est.shift, n, extra_waves, grid_waves, (int)gridDim.x, info, tail, tid);
}

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline uint32_t tile_budget_targets() {  // (laboratory: a wave's budget as this many average targets)
  const int v = lab_int("NBODY_WALK_TILE_BUDGET_TARGETS", 0);
  return (uint32_t)(v < 1 ? 0 : (v > 4096 ? 4096 : v));
}

}  // namespace

WalkSplitLayout walk_split_layout(int64_t n_tgt) {
  WalkSplitLayout L{};
  const size_t n = (size_t)(n_tgt > 0 ? n_tgt : 1);
  size_t o = 0;
  auto take = [&](size_t b) { size_t r = o; o += align_up(b); return r; };
  // first, at the same place whatever n_tgt is (the caller zeroes it once per allocation): walk_scan_est_tail's ticket, epoch
  // and one state per work-group of 1 024 targets, for up to kFusedScanMaxTargets of them
  L.scan_state_bytes = 8 * (kFusedScanMaxTargets / (256 * kScanPer) + 4);
  L.scan_state = take(L.scan_state_bytes);
  L.cnt = take(4 * n);
  L.off = take(4 * n);
  L.info = take(32);
  L.order = take(4 * (size_t)kWalkOrderChunks);
  size_t tb = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, (hipStream_t) nullptr);
  L.cub_temp_bytes = tb;
  L.cub_temp = take(tb);
  L.total = o;
  return L;
}

hipError_t launch_walk_count_scan(hipStream_t s, char* scratch, const WalkSplitLayout& L, int64_t n_tgt) {
  uint32_t* cnt = (uint32_t*)(scratch + L.cnt);
  uint32_t* off = (uint32_t*)(scratch + L.off);
  size_t tb = L.cub_temp_bytes;
  const hipError_t e = hipcub::DeviceScan::ExclusiveSum((void*)(scratch + L.cub_temp), tb, (const uint32_t*)cnt, off, (int)n_tgt, s);
  if (e != hipSuccess) return e;
  walk_check_wrap<<<dim3((unsigned)((n_tgt + 255) / 256)), dim3(256), 0, s>>>(cnt, off, n_tgt, (int*)(scratch + L.info));
  return hipSuccess;
}

// The walk's preparation (the estimate's scan, its wrap check, the waves' budget: info[0..3] are final afterwards) and
// the walk proper, separately: a caller that wants to see info[1] before the long kernel has run enqueues a copy and an
// event between the two.  *grid_waves carries the wave count from the one to the other.
template <class T>
hipError_t launch_tree_walk_tile_prep(hipStream_t s, const WalkArgs<T>& a, char* scratch, const WalkSplitLayout& L, const uint32_t* tgt_ids,
                                      uint32_t* hist, int estimate, int shift, int64_t* grid_waves, const TileTail* tail) {
  const bool have_history = estimate != 0;  // 1: from hist; 2: none at all (every wave takes 64 targets)
  *grid_waves = 0;
  if (tail && (estimate != 1 || a.n_tgt <= 0 || tail->flag_words > 256)) return hipErrorInvalidValue;  // the tail rides on the history estimate's check
  if (a.n_tgt <= 0) return hipSuccess;
  uint32_t* cnt = (uint32_t*)(scratch + L.cnt);
  uint32_t* off = (uint32_t*)(scratch + L.off);
  int* info = (int*)(scratch + L.info);
  hipError_t e = hipSuccess;
  if (!(tail && tail->info_zeroed)) e = hipMemsetAsync(info, 0, 32, s);
  if (e != hipSuccess) return e;
  size_t tb = L.cub_temp_bytes;
  if (!have_history) {  // no counts of an earlier walk over these targets: count (exact, so shift 0)
    shift = 0;
    const int64_t cwaves = (a.n_tgt + kCountTPW - 1) / kCountTPW;
    walk_count<T><<<dim3((unsigned)((cwaves + 3) / 4)), dim3(256), 0, s>>>(a, cnt);
    e = launch_walk_count_scan(s, scratch, L, a.n_tgt);
    if (e != hipSuccess) return e;
  } else if (tail && tail->fused_scan) {
    // (everything is done by the one kernel launched below)
  } else {
    hipcub::CountingInputIterator<int> idx(0);
    hipcub::TransformInputIterator<uint32_t, EstimateOf, hipcub::CountingInputIterator<int>> est(idx, EstimateOf{estimate == 1 ? hist : nullptr, tgt_ids, shift});
    size_t need = 0;  // the layout sized the scan's scratch for plain pointers: make sure this iterator asks for no more
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, est, off, (int)a.n_tgt, s);
    if (e != hipSuccess) return e;
    if (need > tb) return hipErrorInvalidValue;
    e = hipcub::DeviceScan::ExclusiveSum((void*)(scratch + L.cub_temp), tb, est, off, (int)a.n_tgt, s);
    if (e != hipSuccess) return e;
    if (estimate == 1 && !tail)
      walk_check_wrap_est<<<dim3((unsigned)((a.n_tgt + 255) / 256)), dim3(256), 0, s>>>(EstimateOf{hist, tgt_ids, shift}, off, a.n_tgt, info);
  }
  const int ew = lab_int("NBODY_WALK_TILE_WAVES", 0);  // (laboratory: override of tile_waves_target)
  int64_t extra = (ew > 0 ? (int64_t)ew : tile_waves_target(a.n_tgt)) - a.n_tgt / 64;
  if (extra < 256) extra = 256;
  const uint32_t bt = tile_budget_targets();  // development override: a budget of this many average targets
  if (bt) extra = a.n_tgt / bt;
  if (extra < 1) extra = 1;
  const int64_t twaves = extra + a.n_tgt / 64 + 4;  // upper bound of g(t) + 1 (budget >= ceil(total / extra))
  *grid_waves = twaves;
  if (tail && tail->fused_scan && a.n_tgt > kFusedScanMaxTargets) return hipErrorInvalidValue;
  if (tail && tail->fused_scan) {
    const unsigned groups = (unsigned)((a.n_tgt + 256 * kScanPer - 1) / (256 * kScanPer));
    walk_scan_est_tail<<<dim3(groups), dim3(256), 0, s>>>(EstimateOf{hist, tgt_ids, shift}, off, a.n_tgt, (unsigned long long*)(scratch + L.scan_state),
                                                       extra, twaves, info, *tail);
    return hipGetLastError();
  }
  if (tail) {
    int64_t groups = a.n_tgt / 2048;  // (every group ends with an atomic on one counter: few groups, longer loops)
    groups = groups < 32 ? 32 : (groups > 128 ? 128 : groups);
    walk_check_est_tail<<<dim3((unsigned)groups), dim3(256), 0, s>>>(EstimateOf{hist, tgt_ids, shift}, off, a.n_tgt, extra, twaves,
                                                                                      info, *tail);
    return hipGetLastError();
  }
  walk_tile_total<<<dim3(1), dim3(1), 0, s>>>(have_history ? nullptr : cnt, off, a.n_tgt, tgt_ids, estimate == 1 ? hist : nullptr, shift, extra,
                                              twaves, info);
  *grid_waves = twaves;
  return hipGetLastError();
}

template hipError_t launch_tree_walk_tile_prep<float>(hipStream_t, const WalkArgs<float>&, char*, const WalkSplitLayout&, const uint32_t*, uint32_t*, int, int, int64_t*,
                                                      const TileTail*);
template hipError_t launch_tree_walk_tile_prep<double>(hipStream_t, const WalkArgs<double>&, char*, const WalkSplitLayout&, const uint32_t*, uint32_t*, int, int, int64_t*,
                                                       const TileTail*);

}  // namespace nbody
