// The chain of the device-side BVH build (f32, design: bvh_build.hip): the exact sequential sum of a long node's points.
// bvh_chunk_sums and bvh_chunk_runs prepare a long chain chunk by chunk, bvh_big_fold walks it (one work-group per node and
// coordinate).  All of NB_FOLD_TIMING is here.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <cstdio>

#include "bvh_device.h"
#include "bvh_units.h"

namespace nbody {

namespace {

// A window of a node's coordinate.  A scan thread takes 8 consecutive addends: one word of padding after every 8 puts the
// threads of a wave 9 words apart (all 64 banks); the chain reads the window front to back, 8 words at fixed offsets from
// one address.
template <int NT> struct StageView {
  static constexpr int kWords = NT * 9 + 8;
  float* b;
  __device__ __forceinline__ static int at(int e) { return e + (e >> 3); }
  __device__ __forceinline__ float operator[](int e) const { return b[at(e)]; }
};
// s += V[begin .. begin+count) in order, in every lane of every wave that calls (begin, count uniform): all lanes read the
// same LDS word (a broadcast) and add it, 8 clocks per add (node_in_lds below does the same).  No result to hand round.
template <int NT>
__device__ __forceinline__ void chain_run_all(const StageView<NT>& V, int begin, int count, float& s) {
  int e = __builtin_amdgcn_readfirstlane(begin);
  const int end = e + __builtin_amdgcn_readfirstlane(count);
  for (; e < end && (e & 7) != 0; ++e) s = s + V[e];
  if (e + 8 <= end) {  // groups of 8 addends at fixed offsets from one address, the next group in flight
    const float* g = V.b + (e + (e >> 3));
#define NB_CHAIN_LOAD(dst, grp) _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) dst[j_] = g[9 * (grp) + j_];
#define NB_CHAIN_ADD(src) _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) s = s + src[j_]; \
  __builtin_amdgcn_sched_group_barrier(0x100, 8, 0); __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
    float va[8], vb[8];
    NB_CHAIN_LOAD(va, 0)
    for (; e + 24 <= end; e += 16, g += 18) {  // va holds [e, e + 8) here
      NB_CHAIN_LOAD(vb, 1)
      NB_CHAIN_ADD(va)
      NB_CHAIN_LOAD(va, 2)
      NB_CHAIN_ADD(vb)
    }
    if (e + 16 <= end) {
      NB_CHAIN_LOAD(vb, 1)
      NB_CHAIN_ADD(va)
      NB_CHAIN_ADD(vb)
      e += 16;
    } else {
      NB_CHAIN_ADD(va)
      e += 8;
    }
#undef NB_CHAIN_LOAD
#undef NB_CHAIN_ADD
  }
  for (; e < end; ++e) s = s + V[e];
}

// ---- scans over the lanes by DPP (a ds_bpermute per step costs a trip through the LDS pipe) -----------------------------------
// The value CTRL brings to this lane, 0 where it brings none (0, 0 is the identity step).
template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS> __device__ __forceinline__ Step dpp_step(Step v) {
  return Step{dpp_or_zero<CTRL, ROWS>(v.a0), dpp_or_zero<CTRL, ROWS>(v.a1)};
}
// inclusive scan over the wave's 64 lanes, in lane order
__device__ __forceinline__ Step wave_scan_steps(Step v) {
  v = xsum::compose(dpp_step<0x111, 0xf>(v), v);  // row_shr:1
  v = xsum::compose(dpp_step<0x112, 0xf>(v), v);  // row_shr:2
  v = xsum::compose(dpp_step<0x114, 0xf>(v), v);  // row_shr:4
  v = xsum::compose(dpp_step<0x118, 0xf>(v), v);  // row_shr:8
  v = xsum::compose(dpp_step<0x142, 0xa>(v), v);  // row_bcast:15 into rows 1 and 3
  v = xsum::compose(dpp_step<0x143, 0xc>(v), v);  // row_bcast:31 into rows 2 and 3
  return v;
}
// the value of the lane before (wave_shr:1), the identity in lane 0
__device__ __forceinline__ Step wave_prev_step(Step v) { return dpp_step<0x138, 0xf>(v); }

// ---- NW waves working on one node --------------------------------------------------------------------------------
// NW == 1 needs no barrier and no LDS (a wave runs in lock-step); NW > 1 is a whole work-group.
template <int NW> struct Scratch {
  Step w[2][NW];     // wave totals of a scan round; two sets, taken in turn (a round that succeeds has one barrier)
  uint32_t wkind[2][NW];   // per wave: 1 a negative increment, 2 a positive one, 4 a step too large for 32-bit sums
  float redf[2][NW];
  int bad;
  uint32_t bad_s;
};

#ifdef NB_FOLD_TIMING
__device__ unsigned long long g_fold_t[16];
#define NB_FT_ADD(k, v) { if (tid == 0) atomicAdd(&g_fold_t[k], (unsigned long long)(v)); }
#else
#define NB_FT_ADD(k, v)
#endif
// One coordinate (comp 0: x, 1: y) of the fold of bvh_tree.rs:58-61 over P[0, len): min, max, and the sum exactly as
// the sequential chain rounds it.  Every thread of the group returns the same values.  The two coordinates are
// independent chains: they run on different work-groups.
// EPT: consecutive addends per thread and scan (the scan's fixed cost is per thread: more addends each = cheaper).
// chain_off: how many addends of the chain came before P[0] (P may be a window of the node staged in LDS).
template <int NW, int EPT, class Src>
__device__ __forceinline__ void exact_fold(const Src& P, int begin, int len, float s_in, int tid, Scratch<NW>* sh,
                                           float& out_sum, float& out_min, float& out_max, int& stops, int chain_off = 0) {
  // the chain over P[begin, len) (one coordinate), entered with the running sum s_in (0.0 and begin = 0 for a whole node)
  static_assert(NW > 1 && EPT == 8, "a work-group of several waves, a row of the stage per addend of a thread");
  constexpr int TILE = NW * 64 * EPT;
  constexpr int kSmall = 1 << 24;  // wave totals below this: NW of them add up without wrapping
  const int lane = tid & 63, wave = tid >> 6;
  float s = s_in;  // uniform across the group
  float mn = kMaxF, mx = 0.f;
  int pos = begin;
  int par = 0;
  bool seq = false;       // decided from s: a chain at 0.0 is not in any binade yet
  bool foreseen = false;  // the last thing done was a run of real adds up to a crossing that was seen coming
  while (pos < len) {
    Chain ch;
    if (!seq) seq = !xsum::chain_open(s, ch);
    const int gp = chain_off + pos;  // addends behind the chain
    // A chain of same-signed addends leaves its binade about every time the number of addends doubles: near the
    // start of the chain short scans lose less work to the restart than full ones.
    int span = gp > 64 ? gp : 64;
    span = span < TILE ? span : TILE;
    int seq_cnt = gp == 0 ? kChainStart : kSeqRun;
    if (!seq && !foreseen) {
      // ... and where it leaves can be seen coming: gp addends made S ulps, so 2^24 is another gp * (2^24 - S) / S
      // addends away if they go on like that.  The scan stops a little short of that point and real adds carry the
      // chain across (they need no binade), instead of a whole scan failing there and starting over.  A guess: a
      // chain that does something else is scanned and stopped as ever.
      const float rem = (float)gp * ((float)(xsum::kHi<float> - ch.S) / (float)ch.S);
      const int irem = rem < 1.0e9f ? (int)rem : 1000000000;
      const int safe = irem - (irem >> 5) - 8;
      if (safe < 64) {
        seq = true;
        seq_cnt = irem + (irem >> 4) + kSeqRun;
        seq_cnt = seq_cnt < NW * 64 ? seq_cnt : NW * 64;
        foreseen = true;
      } else {
        span = span < safe ? span : safe;
      }
    } else {
      foreseen = false;
    }
    if (seq) {  // real adds, by every wave for itself: nothing to wait for, nothing to pass on
#ifdef NB_FOLD_TIMING
      const long long tq0 = wall_clock64();
#endif
      const int cnt = len - pos < seq_cnt ? len - pos : seq_cnt;
      chain_run_all(P, pos, cnt, s);
      for (int i = tid; i < cnt; i += NW * 64) {
        const float v = P[pos + i];
        mn = sse_min(mn, v);
        mx = sse_max(mx, v);
      }
      pos += cnt;
      seq = false;
#ifdef NB_FOLD_TIMING
      NB_FT_ADD(0, wall_clock64() - tq0) NB_FT_ADD(2, 1)
#endif
      continue;
    }
#ifdef NB_FOLD_TIMING
    const long long tr0 = wall_clock64();
#endif
    const int limit = pos + span < len ? pos + span : len;
    const int base = pos + tid * EPT;
    Step f[EPT];
    Step t = xsum::identity<float>();
    int imin = 0, imax = 0;  // extremes of the increments: their signs, and whether 32-bit totals can be trusted
#pragma unroll
    for (int j = 0; j < EPT; ++j) f[j] = xsum::identity<float>();
    if (base < limit) {
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        if (base + j < limit) {
          const float v = P[base + j];
          f[j] = xsum::step_of(v, ch.sign, ch.E);
          mn = sse_min(mn, v);
          mx = sse_max(mx, v);
          const int i0 = (int)f[j].a0, i1 = (int)f[j].a1;
          imin = min(imin, min(i0, i1));
          imax = max(imax, max(i0, i1));
        }
        t = xsum::compose(t, f[j]);
      }
    }
    const Step inc = wave_scan_steps(t);  // inclusive scan inside the wave
    Step ex = wave_prev_step(inc);        // exclusive: everything before my addends
    {  // (an increment is below 2^22 in size unless it is the poison: 512 of one sign stay below 2^31)
      const uint32_t kind = (__ballot(imin < 0) != 0ull ? 1u : 0u) | (__ballot(imax > 0) != 0ull ? 2u : 0u) |
                            (__ballot(imax >= (1 << 23)) != 0ull ? 4u : 0u);
      if (lane == 63) { sh->w[par][wave] = inc; sh->wkind[par][wave] = kind; }
    }
    if (tid == 0) sh->bad = INT_MAX;
    __syncthreads();
    // every wave scans the NW wave totals for itself (lanes 0..NW-1): no second barrier
    Step wi = xsum::identity<float>();
    uint32_t wk = 0u;
    if (lane < NW) { wi = sh->w[par][lane]; wk = sh->wkind[par][lane]; }
    const int w0 = (int)wi.a0, w1 = (int)wi.a1;
    if (w0 <= -kSmall || w0 >= kSmall || w1 <= -kSmall || w1 >= kSmall) wk |= 4u;
    const uint32_t kind = (__ballot((wk & 1u) != 0u) != 0ull ? 1u : 0u) | (__ballot((wk & 2u) != 0u) != 0ull ? 2u : 0u) |
                          (__ballot((wk & 4u) != 0u) != 0ull ? 4u : 0u);
    static_assert(NW <= 16, "the wave totals are scanned inside one row of 16 lanes");
    wi = xsum::compose(dpp_step<0x111, 0xf>(wi), wi);
    if constexpr (NW > 2) wi = xsum::compose(dpp_step<0x112, 0xf>(wi), wi);
    if constexpr (NW > 4) wi = xsum::compose(dpp_step<0x114, 0xf>(wi), wi);
    if constexpr (NW > 8) wi = xsum::compose(dpp_step<0x118, 0xf>(wi), wi);
    Step tot;
    tot.a0 = (uint32_t)__builtin_amdgcn_readlane((int)wi.a0, NW - 1);
    tot.a1 = (uint32_t)__builtin_amdgcn_readlane((int)wi.a1, NW - 1);
    par ^= 1;
    // Increments of one sign only (the usual case: coordinates of one sign) move S one way: every intermediate S lies
    // between the first and the last, so the last one being inside the binade says all were.  The totals are exact:
    // every wave's is below 2^24 in size, NW of them cannot wrap.
    if (kind != 3u && kind < 4u && xsum::in_binade<float>(xsum::apply(ch.S, tot))) {
      s = xsum::chain_value(ch, xsum::apply(ch.S, tot));
      pos += span;
#ifdef NB_FOLD_TIMING
      NB_FT_ADD(1, wall_clock64() - tr0) NB_FT_ADD(3, 1)
#endif
      continue;
    }
    if (wave > 0) {
      Step pw;  // all the waves before mine
      pw.a0 = (uint32_t)__builtin_amdgcn_readlane((int)wi.a0, wave - 1);
      pw.a1 = (uint32_t)__builtin_amdgcn_readlane((int)wi.a1, wave - 1);
      ex = xsum::compose(pw, ex);
    }
    uint32_t S = xsum::apply(ch.S, ex);
    int bad = INT_MAX;
    uint32_t bs = 0u;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      if (base + j < limit && bad == INT_MAX) {
        const uint32_t nx = xsum::apply(S, f[j]);
        if (!xsum::in_binade<float>(nx)) {
          bad = tid * EPT + j;
          bs = S;
        } else {
          S = nx;
        }
      }
    }
    int first_bad = bad;
    for (int d = 32; d >= 1; d >>= 1) {
      const int o = __shfl_xor(first_bad, d, 64);
      first_bad = o < first_bad ? o : first_bad;
    }
    if (lane == 0 && first_bad != INT_MAX) atomicMin(&sh->bad, first_bad);
    __syncthreads();
    first_bad = sh->bad;
    if (first_bad == INT_MAX) {
      s = xsum::chain_value(ch, xsum::apply(ch.S, tot));
      pos += span;
    } else {  // the chain is exact up to the addend before first_bad; that addend takes a real add
      if (bad == first_bad) sh->bad_s = bs;
      __syncthreads();
      s = xsum::chain_value(ch, sh->bad_s);
      pos += first_bad;
      seq = true;
      ++stops;
    }
    __syncthreads();  // sh->bad, bad_s are rewritten by the next round
#ifdef NB_FOLD_TIMING
    NB_FT_ADD(1, wall_clock64() - tr0) NB_FT_ADD(3, 1) NB_FT_ADD(7, 1)
#endif
  }
  for (int d = 32; d >= 1; d >>= 1) {
    mn = sse_min(mn, __shfl_xor(mn, d, 64));
    mx = sse_max(mx, __shfl_xor(mx, d, 64));
  }
  if (lane == 0) { sh->redf[0][wave] = mn; sh->redf[1][wave] = mx; }
  __syncthreads();
  for (int w = 0; w < NW; ++w) {
    mn = sse_min(mn, sh->redf[0][w]);
    mx = sse_max(mx, sh->redf[1][w]);
  }
  __syncthreads();
  out_sum = s;
  out_min = mn;
  out_max = mx;
}

// exact_fold over P[lo, hi) of a node in memory, a window of NW * 64 * EPT points at a time out of LDS.  The chain is a
// sequence of short dependent rounds (a scan, a stop at every power of two the sum crosses, a few real adds, the next scan):
// read from memory every round pays a trip to L2; the window is fetched once, the next one while this one is folded.
template <int NW, int EPT>
__device__ __forceinline__ void staged_fold(const float2* __restrict__ P, int lo, int hi, float s_in, int comp, int tid,
                                            Scratch<NW>* sh, float* stage, float& out_sum, float& out_min, float& out_max,
                                            int& stops) {
  constexpr int NT = NW * 64, T = NT * EPT;
  const StageView<NT> view{stage};
  const float* __restrict__ X = reinterpret_cast<const float*>(P) + comp;
  float s = s_in, mn = kMaxF, mx = 0.f;
  float nx[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = lo + tid + k * NT;
    nx[k] = e < hi ? X[2 * (size_t)e] : 0.f;
  }
  for (int t0 = lo; t0 < hi; t0 += T) {
    const int cnt = hi - t0 < T ? hi - t0 : T;
    __syncthreads();  // the window before this one has been read to the end
#pragma unroll
    for (int k = 0; k < EPT; ++k) stage[StageView<NT>::at(tid + k * NT)] = nx[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = t0 + T + tid + k * NT;
      nx[k] = e < hi ? X[2 * (size_t)e] : 0.f;
    }
    float ts, tmn, tmx;
    exact_fold<NW, EPT>(view, 0, cnt, s, tid, sh, ts, tmn, tmx, stops, t0);
    s = ts;
    mn = sse_min(mn, tmn);
    mx = sse_max(mx, tmx);
  }
  out_sum = s;
  out_min = mn;
  out_max = mx;
}

// ---- long nodes, one level: chunk sums and chunk runs (only nodes longer than kRunLen) ------------------------------------
// A long chain is cut into chunks of kChunk addends.  bvh_chunk_sums: f64 sums (and the box) of every chunk, in parallel;
// their prefix PREDICTS the binade the chain is in when it reaches a chunk.  bvh_chunk_runs: every chunk's run
// (exact_sum.h) for that binade, in parallel.  bvh_big_fold then walks the chunks: a run is used iff the true state is in
// the predicted binade and the run's bounds hold from it; the other chunks (the first one, the ~log2(len / kChunk) in which
// the sum crosses a power of two, wrong guesses) are added by the scan, as before.
__global__ __launch_bounds__(256) void bvh_chunk_sums(BvhPtrs a, int level) {
  __shared__ double red[6][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nc = a.chunkcount[level];
  const int4* ch_rec = a.ch_rec + (size_t)(level & 1) * a.cap_chunk;
  for (int c = blockIdx.x; c < nc; c += gridDim.x) {
    const int4 cr = ch_rec[c];
    const int ci = cr.y, len = cr.w;
    if (len <= kRunLen) continue;
    const float2* P = a.P + cr.z;
    const int lo = ci * kChunk, hi = lo + kChunk < len ? lo + kChunk : len;
    double sx = 0.0, sy = 0.0;
    Box bx;
    for (int i = lo + tid; i < hi; i += 256) {
      const float2 q = P[i];
      sx += (double)q.x;
      sy += (double)q.y;
      bx.add(q);
    }
    for (int d = 32; d >= 1; d >>= 1) {
      sx += __shfl_xor(sx, d, 64);
      sy += __shfl_xor(sy, d, 64);
    }
    bx.reduce_wave();
    if (lane == 0) {
      red[0][wave] = sx; red[1][wave] = sy;
      red[2][wave] = bx.mnx; red[3][wave] = bx.mny; red[4][wave] = bx.mxx; red[5][wave] = bx.mxy;
    }
    __syncthreads();
    if (tid == 0) {
      double tx = 0.0, ty = 0.0;
      float mnx = kMaxF, mny = kMaxF, mxx = 0.f, mxy = 0.f;
      for (int w = 0; w < 4; ++w) {
        tx += red[0][w]; ty += red[1][w];
        mnx = sse_min(mnx, (float)red[2][w]); mny = sse_min(mny, (float)red[3][w]);
        mxx = sse_max(mxx, (float)red[4][w]); mxy = sse_max(mxy, (float)red[5][w]);
      }
      a.ch_sum[c] = make_double2(tx, ty);
      a.ch_box[c] = make_float4(mnx, mny, mxx, mxy);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ Run shfl_down_run(const Run& r, int d) {
  Run o;
  o.a0 = __shfl_down(r.a0, d, 64); o.a1 = __shfl_down(r.a1, d, 64);
  o.lo0 = __shfl_down(r.lo0, d, 64); o.lo1 = __shfl_down(r.lo1, d, 64);
  o.hi0 = __shfl_down(r.hi0, d, 64); o.hi1 = __shfl_down(r.hi1, d, 64);
  return o;
}

// Runs are prepared per RUN chunk = m consecutive chunks of kChunk addends, m a power of two such that a node has at most
// 64 of them: the chain's walk over the runs is sequential (~0.7 us per run), the preparation is not.
__host__ __device__ inline int run_mult(int len) {
  const int nch = (len + kChunk - 1) / kChunk;
  int m = 1;
  while (nch > 64 * m) m <<= 1;
  return m;
}
constexpr int kGapCap = 2048;  // real adds around powers of two, per chain and walk, fetched ahead into LDS
constexpr int kRunRec = 24;  // ints per chunk and coordinate: sign, E_a (0: no run), E_b, u0, u1, run A (6), run B (6), [17] where its real adds lie in `gaps` (bvh_big_fold), pad
__device__ __forceinline__ void store_run(int* o, const Run& r) {
  o[0] = r.a0; o[1] = r.a1; o[2] = r.lo0; o[3] = r.lo1; o[4] = r.hi0; o[5] = r.hi1;
}
// ordered reduction over the wave: lane 0 ends with r(lane 0) then r(lane 1) then ...
__device__ __forceinline__ Run wave_run_in_order(Run r, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const Run o = shfl_down_run(r, d);
    if ((lane & (2 * d - 1)) == 0) r = xsum::run_then(r, o);
  }
  return r;
}

// One chunk's runs.  Every thread takes PER consecutive addends and the f64 prefix PREDICTS where the chain is at each
// thread.  If the chunk stays in one binade: one run (A) over all of it.  If the prefix crosses ONE power of two B inside
// the chunk (same-signed data): run A (old binade) over the threads safely below B (1 - kRunMargin), run B (new binade)
// over the threads safely above B (1 + kRunMargin), and the threads in between are left to real adds (u0 .. u1).
__global__ __launch_bounds__(256) void bvh_chunk_runs(BvhPtrs a, int level) {
  constexpr int PER = kChunk / 256;
  __shared__ double redd[4][4];
  __shared__ Run redr[2][2][4];  // [coordinate][A / B][wave]
  __shared__ int redi[2][4][4];        // [coordinate][#A, #B, #active, shape ok][wave]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nc = a.chunkcount[level];
  const int4* ch_rec = a.ch_rec + (size_t)(level & 1) * a.cap_chunk;
  for (int c = blockIdx.x; c < nc; c += gridDim.x) {
    const int4 cr = ch_rec[c];
    const int node = cr.x, ci = cr.y, len = cr.w;
    if (len <= kRunLen) continue;
    constexpr int m = 1;  // runs are prepared per chunk; bvh_big_fold merges them into at most 64 per node
    int* rec = a.ch_run + (size_t)c * 2 * kRunRec;
    if (ci == 0) {  // the chain starts here: nothing to predict
      if (tid == 0) { rec[1] = 0; rec[kRunRec + 1] = 0; }
      continue;
    }
    // where the chain should be when it gets here: the f64 sums of the node's chunks before this one
    const int c0 = c - ci;  // a node's chunks are consecutive
    const int nchn = (len + kChunk - 1) / kChunk;
    double px = 0.0, py = 0.0, tx = 0.0, ty = 0.0;
    for (int i = tid; i < ci + m && i < nchn; i += 256) {
      const double2 v = a.ch_sum[c0 + i];
      if (i < ci) { px += v.x; py += v.y; } else { tx += v.x; ty += v.y; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
      px += __shfl_xor(px, d, 64);
      py += __shfl_xor(py, d, 64);
      tx += __shfl_xor(tx, d, 64);
      ty += __shfl_xor(ty, d, 64);
    }
    if (lane == 0) { redd[0][wave] = px; redd[1][wave] = py; redd[2][wave] = tx; redd[3][wave] = ty; }
    __syncthreads();
    px = redd[0][0] + redd[0][1] + redd[0][2] + redd[0][3];
    py = redd[1][0] + redd[1][1] + redd[1][2] + redd[1][3];
    const double2 tot = make_double2(redd[2][0] + redd[2][1] + redd[2][2] + redd[2][3], redd[3][0] + redd[3][1] + redd[3][2] + redd[3][3]);
    __syncthreads();
    const float2* P = a.P + a.nbegin[node] + (size_t)ci * kChunk;               // this run chunk
    const int cnt = (ci + m) * kChunk < len ? m * kChunk : len - ci * kChunk;  // its addends
    const int seg = m * PER;                                                    // consecutive addends per thread
    const int base = tid * seg;
    // does either coordinate cross a power of two in this chunk?  Only then the threads need their own f64 prefix
    Chain cax, cbx, cay, cby;
    const bool hx = xsum::chain_open((float)px, cax) && xsum::chain_open((float)(px + tot.x), cbx) && cax.sign == cbx.sign;
    const bool hy = xsum::chain_open((float)py, cay) && xsum::chain_open((float)(py + tot.y), cby) && cay.sign == cby.sign;
    const bool crossing = (hx && cbx.E == cax.E + 1u) || (hy && cby.E == cay.E + 1u);  // uniform
    double sx0 = 0.0, sy0 = 0.0, lx = 0.0, ly = 0.0;
    if (crossing) {  // f64 prefix of my first addend
      for (int j = 0; j < seg && base + j < cnt; ++j) {
        const float2 qq = P[base + j];
        lx += (double)qq.x;
        ly += (double)qq.y;
      }
      double ix = lx, iy = ly;
      for (int d = 1; d < 64; d <<= 1) {
        const double ox = __shfl_up(ix, d, 64), oy = __shfl_up(iy, d, 64);
        if (lane >= d) { ix += ox; iy += oy; }
      }
      if (lane == 63) { redd[0][wave] = ix; redd[1][wave] = iy; }
      __syncthreads();
      sx0 = px + ix - lx;
      sy0 = py + iy - ly;
      for (int w = 0; w < wave; ++w) { sx0 += redd[0][w]; sy0 += redd[1][w]; }
    }
    const bool active = base < cnt;
    for (int comp = 0; comp < 2; ++comp) {
      const double s0 = comp ? sy0 : sx0, s1 = s0 + (comp ? ly : lx);
      const Chain ca = comp ? cay : cax, cb = comp ? cby : cbx;
      const bool have = (comp ? hy : hx) && (cb.E == ca.E || cb.E == ca.E + 1u);
      int cls = 2;  // 0: run A, 1: run B, 2: left to real adds
      if (have) {
        if (cb.E == ca.E) {
          cls = 0;
        } else {
          const double sgn = ca.sign ? -1.0 : 1.0;
          const double B = __builtin_ldexp(1.0, (int)cb.E - 127);
          const double lo = B * (1.0 - xsum::kRunMargin), hi = B * (1.0 + xsum::kRunMargin);
          const double qs = sgn * s0, qe = sgn * s1;
          if (qs < lo && qe < lo) cls = 0;
          else if (qs > hi && qe > hi) cls = 1;
        }
      }
      if (!active) cls = 3;
      const unsigned long long mA = __builtin_amdgcn_ballot_w64(cls == 0), mB = __builtin_amdgcn_ballot_w64(cls == 1);
      const unsigned long long mAct = __builtin_amdgcn_ballot_w64(active);
      if (lane == 0) {  // inside the wave: A threads first, B threads last (the active threads are a prefix of the lanes)
        const int nA = __builtin_popcountll(mA), nB = __builtin_popcountll(mB), nAct = __builtin_popcountll(mAct);
        const unsigned long long lowA = nA >= 64 ? ~0ull : ((1ull << nA) - 1ull);
        const unsigned long long lowNB = (nAct - nB) >= 64 ? ~0ull : ((1ull << (nAct - nB)) - 1ull);
        redi[comp][0][wave] = nA;
        redi[comp][1][wave] = nB;
        redi[comp][2][wave] = nAct;
        redi[comp][3][wave] = (mA == lowA && mB == (mAct & ~lowNB)) ? 1 : 0;
      }
      Run r = xsum::run_none<float>();
      if (cls == 0 || cls == 1) {
        const Chain& ch = cls ? cb : ca;
        for (int j = 0; j < seg && base + j < cnt; ++j) {
          const float2 qq = P[base + j];
          r = xsum::run_then(r, xsum::run_of(xsum::step_of(comp ? qq.y : qq.x, ch.sign, ch.E)));
        }
      }
      // ordered reduction: a wave is usually all A or all B; only a wave that straddles the crossing reduces twice
      Run ra = xsum::run_none<float>(), rb = xsum::run_none<float>();
      if (mB == 0ull) {
        ra = wave_run_in_order(cls == 0 ? r : xsum::run_none<float>(), lane);
      } else if (mA == 0ull) {
        rb = wave_run_in_order(cls == 1 ? r : xsum::run_none<float>(), lane);
      } else {
        ra = wave_run_in_order(cls == 0 ? r : xsum::run_none<float>(), lane);
        rb = wave_run_in_order(cls == 1 ? r : xsum::run_none<float>(), lane);
      }
      if (lane == 0) { redr[comp][0][wave] = ra; redr[comp][1][wave] = rb; }
      __syncthreads();
      if (tid == 0) {
        int* o = rec + comp * kRunRec;
        int nA = 0, nB = 0, nAct = 0;
        for (int w = 0; w < 4; ++w) { nA += redi[comp][0][w]; nB += redi[comp][1][w]; nAct += redi[comp][2][w]; }
        // A must be a prefix of the chunk's threads and B a suffix (same-signed data, one crossing)
        bool ok = have;
        bool a_over = false, b_begun = false;
        for (int w = 0; w < 4; ++w) {
          const int wa = redi[comp][0][w], wb = redi[comp][1][w], wact = redi[comp][2][w];
          if (!redi[comp][3][w]) ok = false;
          if (a_over && wa > 0) ok = false;
          if (b_begun && wb != wact) ok = false;
          if (wa < wact) a_over = true;
          if (wb > 0) b_begun = true;
        }
        o[0] = (int)ca.sign;
        o[1] = ok ? (int)ca.E : 0;
        o[2] = (int)cb.E;
        const int u0 = nA * seg < cnt ? nA * seg : cnt;
        const int u1 = (nAct - nB) * seg < cnt ? (nAct - nB) * seg : cnt;
        o[3] = u0;
        o[4] = u1 > u0 ? u1 : u0;
        Run A = redr[comp][0][0], Bq = redr[comp][1][0];
        for (int w = 1; w < 4; ++w) { A = xsum::run_then(A, redr[comp][0][w]); Bq = xsum::run_then(Bq, redr[comp][1][w]); }
        store_run(o + 5, A);
        store_run(o + 11, Bq);
      }
      __syncthreads();
    }
  }
}

// ---- long nodes, one level: fold ---------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void bvh_big_fold(BvhPtrs a, int level, int use_runs) {
  constexpr int kRecBatch = 64;
  __shared__ Scratch<8> sh;
  __shared__ __attribute__((aligned(16))) int recs[kRecBatch * kRunRec];
  __shared__ float stage[StageView<512>::kWords];
  __shared__ float gaps[kGapCap];
  __shared__ int gap_total;
  const int tid = threadIdx.x;
  const int comp = blockIdx.y;  // 0: x, 1: y
  const int nq = a.bigcount[level];
  const int* queue = a.bigq + (size_t)(level & 1) * a.cap_big;
  int stops = 0;
  for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
    const int node = queue[qi];
    const int b = a.nbegin[node], len = a.nlen[node];
    const float2* P = (const float2*)(a.P + b);
    float sum, mn, mx;
#ifdef NB_FOLD_TIMING
    const long long tn0 = wall_clock64();
#endif
    if (use_runs && len > kRunLen) {
      const int c0 = a.nchunk0[node], nch = (len + kChunk - 1) / kChunk;
      const int rm = run_mult(len), rlen = rm * kChunk, nrun = (nch + rm - 1) / rm;  // run chunks: <= 64 of them
      sum = 0.f;
      int used = 0;
      {  // the chunks' runs are merged, rm at a time, into the <= 64 runs the chain will walk (one thread per merged run)
        const int b0 = 0, nb = nrun;
        int glen = 0;
#ifdef NB_FOLD_TIMING
        long long tr0 = wall_clock64();
#endif
        if (tid < nrun) {
          const int f0 = tid * rm, f1 = f0 + rm < nch ? f0 + rm : nch;
          Run A = xsum::run_none<float>(), B = xsum::run_none<float>();
          int sign = 0, Ea = 0, Eb = 0, u0 = 0, u1 = 0, pos = 0;
          bool valid = true, crossed = false;
          for (int f = f0; f < f1 && valid; ++f) {
            const int* fr = a.ch_run + (size_t)(c0 + f) * 2 * kRunRec + comp * kRunRec;
            const int cntf = (f + 1) * kChunk < len ? kChunk : len - f * kChunk;
            const int fE = fr[1];
            if (fE == 0) { valid = false; break; }
            Run fa, fb;
            fa.a0 = fr[5]; fa.a1 = fr[6]; fa.lo0 = fr[7]; fa.lo1 = fr[8]; fa.hi0 = fr[9]; fa.hi1 = fr[10];
            fb.a0 = fr[11]; fb.a1 = fr[12]; fb.lo0 = fr[13]; fb.lo1 = fr[14]; fb.hi0 = fr[15]; fb.hi1 = fr[16];
            const bool whole = fr[3] >= cntf;  // one run over the whole chunk
            if (f == f0) { sign = fr[0]; Ea = fE; Eb = fE; }
            if (fr[0] != sign) { valid = false; break; }
            if (!crossed) {
              if (fE != Ea) { valid = false; break; }
              A = xsum::run_then(A, fa);
              if (!whole) {  // the power of two falls into this chunk
                u0 = pos + fr[3];
                u1 = pos + fr[4];
                B = fb;
                Eb = fr[2];
                crossed = true;
              }
            } else {
              if (fE != Eb || !whole) { valid = false; break; }  // a second crossing: leave it to the scan
              B = xsum::run_then(B, fa);
            }
            pos += cntf;
          }
          if (!crossed) { u0 = pos; u1 = pos; }
          int* o = recs + tid * kRunRec;
          o[0] = sign; o[1] = valid ? Ea : 0; o[2] = Eb; o[3] = u0; o[4] = u1;
          o[5] = A.a0; o[6] = A.a1; o[7] = A.lo0; o[8] = A.lo1; o[9] = A.hi0; o[10] = A.hi1;
          o[11] = B.a0; o[12] = B.a1; o[13] = B.lo0; o[14] = B.lo1; o[15] = B.hi0; o[16] = B.hi1;
          glen = valid ? u1 - u0 : 0;  // addends around a power of two, left to real adds
        }
        if (tid < 64) {
          // Those addends are fetched for all runs at once, ahead of the walk (a trip to memory at every crossing is 2 us
          // of a walk that takes 0.1 us per run): where each run's lie in `gaps` (nrun <= 64: the merging threads are
          // this wave).  Runs whose addends do not fit are left to the scan.
          int inc = glen;
          for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if ((tid & 63) >= d) inc += o;
          }
          const int goff = inc - glen;
          if (tid < nrun) {
            int* o = recs + tid * kRunRec;
            o[17] = goff;
            if (goff + glen > kGapCap) o[1] = 0;
#ifdef NB_FORCE_SCANS
            if ((tid % NB_FORCE_SCANS) == 1) o[1] = 0;  // (test builds) every so many runs go to the scan instead
#endif
          }
          if (tid == 63) gap_total = inc < kGapCap ? inc : kGapCap;
        }
        __syncthreads();
#ifdef NB_FOLD_TIMING
        { const long long t = wall_clock64(); NB_FT_ADD(8, t - tr0) tr0 = t; }
#endif
        {
          const float* __restrict__ X = reinterpret_cast<const float*>(P) + comp;
          const int G = gap_total;
          for (int g = tid; g < G; g += 512) {
            int lo_r = 0, hi_r = nrun - 1;  // the run whose addends include the g-th: last one with offset <= g
            while (lo_r < hi_r) {
              const int mid = (lo_r + hi_r + 1) >> 1;
              if (recs[mid * kRunRec + 17] <= g) lo_r = mid; else hi_r = mid - 1;
            }
            const int* o = recs + lo_r * kRunRec;
            const int k = g - o[17];
            if (o[1] != 0 && k < o[4] - o[3]) gaps[g] = X[2 * (size_t)(lo_r * rlen + o[3] + k)];
          }
        }
        __syncthreads();
#ifdef NB_FOLD_TIMING
        { const long long t = wall_clock64(); NB_FT_ADD(9, t - tr0) NB_FT_ADD(13, gap_total) tr0 = t; }
#endif
        int ci = b0;
        while (ci < b0 + nb) {  // ... and the chain walks through them in order
          // one wave runs ahead as long as the prepared runs hold (a few dozen instructions per chunk, no barrier) ...
          if (tid < 64) {
            // The chain's state stays (sign, E, S) from run to run; it turns into a float only where real adds need one.
            Chain ch;
            bool open = xsum::chain_open(sum, ch);
            for (; ci < b0 + nb; ++ci) {
              // the whole record in one go (LDS latency once per chunk, not once per field)
              const int4* rv = reinterpret_cast<const int4*>(recs + (ci - b0) * kRunRec);
              const int4 r0 = rv[0], r1 = rv[1], r2 = rv[2], r3 = rv[3], r4 = rv[4];
              if (r0.y == 0 || !open) break;  // no run prepared, or a state no run applies to: the scan's
              const int lo = ci * rlen, hi = lo + rlen < len ? lo + rlen : len;
              const int u0 = r0.w, u1 = r1.x;
              Chain tc = ch;
              bool good = true;
              int u = 0;
              if (u0 > 0) {  // part A: [lo, lo + u0)
                Run r;
                r.a0 = r1.y; r.a1 = r1.z; r.lo0 = r1.w; r.lo1 = r2.x; r.hi0 = r2.y; r.hi1 = r2.z;
                good = (int)tc.E == r0.y && (int)tc.sign == r0.x && xsum::run_fits(tc.S, r);
                tc.S = (uint32_t)((int)tc.S + ((tc.S & 1u) ? r.a1 : r.a0));
                ++u;
              }
              if (good && u1 > u0) {  // the addends around the power of two: real adds, out of `gaps`
                float t = xsum::chain_value(tc, tc.S);
                t = chain_lds<1>(gaps + r4.y, u1 - u0, t);
                good = xsum::chain_open(t, tc);
              }
              if (good && lo + u1 < hi) {  // part B: [lo + u1, hi), in the binade above
                good = (int)tc.E == r0.z && (int)tc.sign == r0.x;
                Run r;
                r.a0 = r2.w; r.a1 = r3.x; r.lo0 = r3.y; r.lo1 = r3.z; r.hi0 = r3.w; r.hi1 = r4.x;
                good = good && xsum::run_fits(tc.S, r);
                tc.S = (uint32_t)((int)tc.S + ((tc.S & 1u) ? r.a1 : r.a0));
                ++u;
              }
              if (!good) break;  // ... a chunk whose run does not hold is everybody's business
              ch = tc;
              used += u;
            }
            if (open) sum = xsum::chain_value(ch, ch.S);
            if (tid == 0) { sh.bad_s = xsum::to_bits(sum); sh.bad = ci; }
          }
          __syncthreads();
#ifdef NB_FOLD_TIMING
          { const long long t = wall_clock64(); NB_FT_ADD(10, t - tr0) tr0 = t; }
#endif
          sum = xsum::from_bits<float>(sh.bad_s);
          ci = sh.bad;
          __syncthreads();
          if (ci >= b0 + nb) break;
          {  // this chunk by the scan, from the true state (its first part may still be taken whole)
            const int* rec = recs + (ci - b0) * kRunRec;
            const int lo = ci * rlen, hi = lo + rlen < len ? lo + rlen : len;
            float dmn, dmx;
            staged_fold<8, 8>(P, lo, hi, sum, comp, tid, &sh, stage, sum, dmn, dmx, stops);
            (void)rec;
            ++ci;
#ifdef NB_FOLD_TIMING
            { const long long t = wall_clock64(); NB_FT_ADD(11, t - tr0) NB_FT_ADD(12, 1) tr0 = t; }
#endif
          }
        }
        __syncthreads();
      }
      mn = kMaxF;
      mx = 0.f;
      for (int ci = tid; ci < nch; ci += 512) {
        const float4 bx = a.ch_box[c0 + ci];
        mn = sse_min(mn, comp ? bx.y : bx.x);
        mx = sse_max(mx, comp ? bx.w : bx.z);
      }
      for (int d = 32; d >= 1; d >>= 1) {
        mn = sse_min(mn, __shfl_xor(mn, d, 64));
        mx = sse_max(mx, __shfl_xor(mx, d, 64));
      }
      if ((tid & 63) == 0) { sh.redf[0][tid >> 6] = mn; sh.redf[1][tid >> 6] = mx; }
      __syncthreads();
      for (int w = 0; w < 8; ++w) {
        mn = sse_min(mn, sh.redf[0][w]);
        mx = sse_max(mx, sh.redf[1][w]);
      }
      __syncthreads();
      if (tid == 0 && used) atomicAdd(&a.flags[kBvhRunsUsed], used);
    } else {
      staged_fold<8, 8>(P, 0, len, 0.f, comp, tid, &sh, stage, sum, mn, mx, stops);
    }
#ifdef NB_FOLD_TIMING
    NB_FT_ADD(4, wall_clock64() - tn0) NB_FT_ADD(5, 1) NB_FT_ADD(6, len)
#endif
    if (tid == 0) {
      float* box = (float*)&a.nbox[node];
      box[comp] = mn;
      box[2 + comp] = mx;
      ((float*)&a.nmean[node])[comp] = sum / (float)len;  // :67
    }
  }
  if (tid == 0 && stops) atomicAdd(&a.flags[kBvhStops], stops);
}

}  // namespace

void launch_bvh_chunk_sums(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level) {
  bvh_chunk_sums<<<dim3((unsigned)gc), dim3(256), 0, s>>>(make_ptrs(scratch, L), level);
}
void launch_bvh_chunk_runs(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level) {
  bvh_chunk_runs<<<dim3((unsigned)gc), dim3(256), 0, s>>>(make_ptrs(scratch, L), level);
}

#ifdef NB_FOLD_TIMING
static void bvh_debug_fold_times(hipStream_t s) {
  unsigned long long h[16] = {};
  (void)hipStreamSynchronize(s);
  (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fold_t), sizeof(h));
  std::fprintf(stderr, "[fold timing, 10 ns ticks] seq %llu in %llu runs; scan %llu in %llu rounds; nodes %llu ticks over %llu chains, %llu points; %llu slow rounds\n",
               h[0], h[2], h[1], h[3], h[4], h[5], h[6], h[7]);
  if (h[8] | h[9] | h[10] | h[11])
    std::fprintf(stderr, "    run path: merge %llu, gap fetch %llu (%llu addends), run walks %llu, scanned chunks %llu in %llu\n", h[8], h[9], h[13], h[10], h[11], h[12]);
  unsigned long long z[16] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_fold_t), z, sizeof(z));
}
#endif
void launch_bvh_big_fold(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gb, int level, int use_runs) {
  bvh_big_fold<<<dim3((unsigned)gb, 2), dim3(512), 0, s>>>(make_ptrs(scratch, L), level, use_runs);
#ifdef NB_FOLD_TIMING
  std::fprintf(stderr, "level %d: ", level);
  bvh_debug_fold_times(s);
#endif
}


}  // namespace nbody
