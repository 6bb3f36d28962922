// What the units of the big-leaf BVH walk share on the device (walk_prepare.hip, walk_tile.hip, walk_tile_fast.hip, walk_lab.hip):
// the budget constants, a pair's term in both precisions and both arithmetics, which targets a wave takes, and the DPP /
// permlane reductions of the FAST walks.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "div_pair.h"
#include "tree_kernels.h"

namespace nbody {

// Targets per wave.  Counting is cheapest with full waves; in the term pass a wave's time grows with the number of
// leaves its targets visit, so its waves are cut by work (see walk_pass).
constexpr int kCountTPW = 64;
[[maybe_unused]] constexpr uint32_t kTermBudget = 8192;  // (three-pass walk, laboratory build) terms a wave of the term pass writes, about (at least: see walk_total)
[[maybe_unused]] constexpr uint32_t kBudgetTargets = 12; // ... or this many average targets' worth, if that is more
constexpr uint32_t kTileBudget = 8192;        // smallest budget of a wave of the one-pass walk (walk_tile)
#ifndef NB_TILE_ROUND_COST
#define NB_TILE_ROUND_COST 66
#endif
#ifndef NB_FAST_ROUND_COST
#define NB_FAST_ROUND_COST 19
#endif
// Which group of four waves a work-group takes (WalkArgs::block_stride).
__device__ __forceinline__ unsigned group_of_block(unsigned b, unsigned nb, int stride) {
  return stride > 1 ? (unsigned)(((unsigned long long)b * (unsigned)stride) % nb) : b;
}
template <class T> __device__ __forceinline__ unsigned group_of_block(const WalkArgs<T>& a, unsigned b, unsigned nb) {
  if (a.group_order) {  // chunk by chunk, the chunks heaviest first (walk_order_chunks); inside a chunk in order (tree-order neighbours share their L2 lines)
    const unsigned slot = b / (unsigned)a.order_chunk;
    return (unsigned)a.group_order[slot] * (unsigned)a.order_chunk + (b - slot * (unsigned)a.order_chunk);
  }
  return group_of_block(b, nb, a.block_stride);
}
constexpr int kTileRoundCost = NB_TILE_ROUND_COST;  // instructions a target costs at a leaf, lane = particle (a round + its share of the adds)
constexpr int kFusedPairCost = 48;            // ... and a particle costs the wave, lane = target

__device__ __forceinline__ float lane_f(float v, int k) {  // k uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}

// calculate_gravity (main.rs:234-253) up to, but not including, the `+=`
__device__ __forceinline__ float2 pair_term(float px, float py, float qx, float qy, float force, float clamp) {
  const float dx = qx - px;                                        // :236
  const float dy = qy - py;
  const float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);     // :238
  if (!__builtin_isnormal(sum)) return make_float2(-0.0f, -0.0f);  // :241-243: no addition at all == adding -0.0
  float distance = dx * dx + dy * dy;                              // :245
  // :247-249 `if distance < 0.001 { distance = 0.001 }` as one v_max_f32 (half the cost of compare + select): `distance`
  // is never NaN here (a normal `sum` means finite dx, dy), and for a NaN clamp both forms keep `distance`
  distance = __builtin_fmaxf(distance, clamp);
  const float den = sum * distance;
  return div_pair(dx * force, dy * force, den);                    // :252 (div_pair.h: the two quotients, packed)
}
// The same with a per-lane `valid` folded into the skip: a lane past the leaf's end yields -0.0 like a skipped pair, under
// the one exec mask (a select afterwards costs two v_cndmask per round).
__device__ __forceinline__ float2 pair_term_if(bool valid, float px, float py, float qx, float qy, float force, float clamp) {
  const float dx = qx - px;
  const float dy = qy - py;
  const float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
  if (!(valid && __builtin_isnormal(sum))) return make_float2(-0.0f, -0.0f);
  float distance = dx * dx + dy * dy;
  distance = __builtin_fmaxf(distance, clamp);
  const float den = sum * distance;
  return div_pair(dx * force, dy * force, den);
}

// ... and as straight-line code: the term computed for every lane, kept by a select (the quotients of a skipped pair are whatever
// the division makes of its operands and are thrown away).  No exec region, so the rounds of two targets sit in ONE basic block.
// (The two rounds written as packed ops over the two targets — subtractions, squares, denominators, numerators and the divisions'
// multiply-adds — are bit-identical too and measured SLOWER: 66 VGPRs instead of 60, seven waves per SIMD, Plummer 1 M 5.70 -> 6.00 ms.)
__device__ __forceinline__ float2 pair_term_sel(bool valid, float px, float py, float qx, float qy, float force, float clamp) {
  const float dx = qx - px;
  const float dy = qy - py;
  const float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
  const bool ok = valid & __builtin_isnormal(sum);
  const float distance = __builtin_fmaxf(dx * dx + dy * dy, clamp);
  const float den = sum * distance;
  const float2 t = div_pair(dx * force, dy * force, den);
  return make_float2(ok ? t.x : -0.0f, ok ? t.y : -0.0f);
}

// nbody_arith FAST (opt-in, tolerance instead of bit parity): one reciprocal instead of two IEEE divisions; a zero difference
// contributes exactly 0 through the biased denominator (direct_kernels.hip)
[[maybe_unused]] __device__ __forceinline__ float2 pair_term_fast(float px, float py, float qx, float qy, float force, float clamp) {
  const float dx = qx - px, dy = qy - py;
  const float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
  const float d2 = __builtin_fmaxf(__builtin_fmaf(dy, dy, dx * dx), clamp);
  const float s = force * __builtin_amdgcn_rcpf(__builtin_fmaf(sum, d2, 8.0779356694631609e-28f));  // 2^-90
  return make_float2(dx * s, dy * s);
}
template <bool FAST> __device__ __forceinline__ float2 term_of(float px, float py, float qx, float qy, float force, float clamp) {
  if constexpr (FAST) return pair_term_fast(px, py, qx, qy, force, clamp);
  else return pair_term(px, py, qx, qy, force, clamp);
}

// ---- the same pieces for either precision (walk_tile) ---------------------------------------------------------------
template <class T> struct Vec2Of;
template <> struct Vec2Of<float> { using type = float2; };
template <> struct Vec2Of<double> { using type = double2; };
template <class T> struct Vec4Of;
template <> struct Vec4Of<float> { using type = float4; };
template <> struct Vec4Of<double> { using type = double4; };
__device__ __forceinline__ float lane_t(float v, int k) { return lane_f(v, k); }
__device__ __forceinline__ double lane_t(double v, int k) {  // k uniform
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, k), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), k);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double2 pair_term(double px, double py, double qx, double qy, double force, double clamp) {
  const double dx = qx - px;                                       // main.rs:236
  const double dy = qy - py;
  const double sum = __builtin_fabs(dx) + __builtin_fabs(dy);      // :238
  if (!__builtin_isnormal(sum)) return make_double2(-0.0, -0.0);   // :241-243
  double distance = dx * dx + dy * dy;                             // :245
  distance = __builtin_fmax(distance, clamp);                      // :247-249 (see the f32 version)
  const double den = sum * distance;
  return make_double2((dx * force) / den, (dy * force) / den);     // :252
}
__device__ __forceinline__ double2 pair_term_if(bool valid, double px, double py, double qx, double qy, double force, double clamp) {
  const double dx = qx - px;
  const double dy = qy - py;
  const double sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  if (!(valid && __builtin_isnormal(sum))) return make_double2(-0.0, -0.0);
  double distance = dx * dx + dy * dy;
  distance = __builtin_fmax(distance, clamp);
  const double den = sum * distance;
  return make_double2((dx * force) / den, (dy * force) / den);
}
__device__ __forceinline__ double2 pair_term_sel(bool valid, double px, double py, double qx, double qy, double force, double clamp) {
  const double dx = qx - px;
  const double dy = qy - py;
  const double sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  const bool ok = valid & __builtin_isnormal(sum);
  const double distance = __builtin_fmax(dx * dx + dy * dy, clamp);
  const double den = sum * distance;
  const double tx = (dx * force) / den, ty = (dy * force) / den;
  return make_double2(ok ? tx : -0.0, ok ? ty : -0.0);
}
__device__ __forceinline__ double2 pair_term_fast(double px, double py, double qx, double qy, double force, double clamp) {
  const double dx = qx - px, dy = qy - py;
  const double sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  const double d2 = __builtin_fmax(__builtin_fma(dy, dy, dx * dx), clamp);
  const double den = __builtin_fma(sum, d2, 0x1p-700);
  double r = __builtin_amdgcn_rcp(den);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  const double sc = force * r;
  return make_double2(dx * sc, dy * sc);
}
template <bool FAST> __device__ __forceinline__ double2 term_of(double px, double py, double qx, double qy, double force, double clamp) {
  if constexpr (FAST) return pair_term_fast(px, py, qx, qy, force, clamp);
  else return pair_term(px, py, qx, qy, force, clamp);
}
template <class T> __device__ __forceinline__ typename Vec2Of<T>::type neg_zero2() {
  typename Vec2Of<T>::type v;
  v.x = (T)-0.0;
  v.y = (T)-0.0;
  return v;
}

// Which targets are wave w's: those with g(t) = off[t] / budget + t / 64 == w (g is non-decreasing): [t0, t1).  A 64-ARY search —
// every lane probes one point of the range, a ballot finds the first that has reached w — narrows 64-fold per round trip: three
// rounds for 151 405 targets and ONE for the second bound (t1 <= t0 + 64), instead of the forty dependent probes of two binary
// searches (16 us of every wave's start, on the scalar side; 125 us as vector loads with a division each before that).
// off / budget as a multiply-high by M = floor((2^32 - 1) / budget): monotone in `off`, never above the true quotient, the same
// integer for every wave — all that g needs.  The budget is then ANY integer (round 4: a power of two left the wave count anywhere
// between the aim and half of it, and the walk's time follows the wave count: profiles/r04_walk_wave_target.txt).
__device__ __forceinline__ int off_quot(uint32_t off, uint32_t M) { return (int)__umulhi(off, M); }
__device__ __forceinline__ void wave_targets(const uint32_t* __restrict__ off, const int n_tgt, const int wave, const uint32_t M, const int lane,
                                             int& t0, int& t1) {
  int lo = 0, hi = n_tgt;  // the first t with g(t) >= wave lies in [lo, hi] (hi = "none below hi")
  while (lo < hi) {
    const int step = (hi - lo + 63) >> 6;
    const int idx = lo + lane * step;
    const bool reached = idx >= hi || off_quot(off[idx], M) + (idx >> 6) >= wave;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(reached);
    const int first = m ? __builtin_ctzll(m) : 64;  // (lane 0 probes lo itself)
    if (first == 0) { hi = lo; break; }
    const int below = lo + (first - 1) * step;      // the last probe that has not reached `wave`
    if (first < 64) hi = min(hi, lo + first * step);
    lo = below + 1;
  }
  t0 = lo;
  const int idx = t0 + lane;                        // the first t with g(t) > wave: at most 64 further on
  const bool past = idx >= n_tgt || off_quot(off[idx], M) + (idx >> 6) > wave;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(past);
  t1 = t0 + (m ? __builtin_ctzll(m) : 64);
  if (t1 > n_tgt) t1 = n_tgt;
}

constexpr int kFastRoundCost = NB_FAST_ROUND_COST;  // VALU instructions a target costs at a leaf, lane = particle (round + its share of the reduction)
constexpr int kFastPairCost = 14;   // ... and a particle costs the wave, lane = target (three broadcasts, the pair, two FMAs)

// v_permlane32_swap / v_permlane16_swap (new in gfx950) through inline asm: this compiler's __builtin_amdgcn_permlane32_swap
// hands back element 0 of the result pair twice (its lowering extracts value 0 for both halves), so the second register
// of the swap is lost.  The s_nop covers "VALU writes a VGPR, a permlane swap reads it: two wait states", which the
// compiler inserts for its own instructions and cannot see inside an asm; what reads the results next is a plain add.
//   swap_halves: a <- {a.lo, b.lo}, b <- {a.hi, b.hi} (halves of 32 lanes)
//   swap_rows:   a <- {a.r0, b.r0, a.r2, b.r2}, b <- {a.r1, b.r1, a.r3, b.r3} (rows of 16 lanes)
__device__ __forceinline__ void swap_halves(float& a, float& b) {
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void swap_rows(float& a, float& b) {
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
[[maybe_unused]] __device__ __forceinline__ void swap_halves(double& a, double& b) {
  unsigned long long ua = __builtin_bit_cast(unsigned long long, a), ub = __builtin_bit_cast(unsigned long long, b);
  unsigned al = (unsigned)ua, ah = (unsigned)(ua >> 32), bl = (unsigned)ub, bh = (unsigned)(ub >> 32);
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3" : "+v"(al), "+v"(ah), "+v"(bl), "+v"(bh));
  a = __builtin_bit_cast(double, ((unsigned long long)ah << 32) | al);
  b = __builtin_bit_cast(double, ((unsigned long long)bh << 32) | bl);
}
[[maybe_unused]] __device__ __forceinline__ void swap_rows(double& a, double& b) {
  unsigned long long ua = __builtin_bit_cast(unsigned long long, a), ub = __builtin_bit_cast(unsigned long long, b);
  unsigned al = (unsigned)ua, ah = (unsigned)(ua >> 32), bl = (unsigned)ub, bh = (unsigned)(ub >> 32);
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3" : "+v"(al), "+v"(ah), "+v"(bl), "+v"(bh));
  a = __builtin_bit_cast(double, ((unsigned long long)ah << 32) | al);
  b = __builtin_bit_cast(double, ((unsigned long long)bh << 32) | bl);
}
// v as the DPP control CTRL moves it (every source lane lies inside the row: nothing is out of range)
template <int CTRL, int BANKS = 0xf> __device__ __forceinline__ float dpp_of(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xf, BANKS, BANKS == 0xf));
}
template <int CTRL, int BANKS = 0xf> __device__ __forceinline__ double dpp_of(double old, double v) {
  const unsigned long long uo = __builtin_bit_cast(unsigned long long, old), uv = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)uo, (int)(unsigned)uv, CTRL, 0xf, BANKS, BANKS == 0xf);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(uo >> 32), (int)(unsigned)(uv >> 32), CTRL, 0xf, BANKS, BANKS == 0xf);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
constexpr int kDppRor8 = 0x128, kDppHalfMirror = 0x141, kDppQuad1032 = 0xB1, kDppQuad2301 = 0x4E, kDppQuadIdentity = 0xE4;
// the sum over 8 consecutive lanes, in every one of them
template <class T> __device__ __forceinline__ T sum_of_8_lanes(T r) {
  r = r + dpp_of<kDppHalfMirror>((T)0, r);
  r = r + dpp_of<kDppQuad1032>((T)0, r);
  r = r + dpp_of<kDppQuad2301>((T)0, r);
  return r;
}
// Eight values per lane -> the 64-lane total of value k in the 8 lanes from kSlotLane8(k) on.
__device__ __forceinline__ int slot_lane8(int k) { return 16 * (((k & 1) << 1) | ((k >> 1) & 1)) + 8 * (k >> 2); }  // row {0,2,1,3}[k & 3], half-row k >> 2
template <class T> __device__ __forceinline__ T reduce8(T (&v)[8]) {
  T p[4], q[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // half h of p[j]: value 2j + h summed over the two halves
    swap_halves(v[2 * j], v[2 * j + 1]);
    p[j] = v[2 * j] + v[2 * j + 1];
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // row r of q[i]: value 4i + {0,2,1,3}[r] summed over four rows
    swap_rows(p[2 * i], p[2 * i + 1]);
    q[i] = p[2 * i] + p[2 * i + 1];
  }
  const T a = q[0] + dpp_of<kDppRor8>((T)0, q[0]);   // lanes i and i ^ 8 of a row added
  const T b = q[1] + dpp_of<kDppRor8>((T)0, q[1]);
  const T r = dpp_of<kDppQuadIdentity, 0xc>(a, b);   // lanes 0-7 of every row keep a (values 0-3), lanes 8-15 take b (values 4-7)
  return sum_of_8_lanes(r);
}
// Four values per lane -> the total of value k in the 16 lanes of row {0,2,1,3}[k].
template <class T> __device__ __forceinline__ T reduce4(T (&v)[4]) {
  swap_halves(v[0], v[1]);
  swap_halves(v[2], v[3]);
  T w0 = v[0] + v[1], w1 = v[2] + v[3];
  swap_rows(w0, w1);
  T u = w0 + w1;
  u = u + dpp_of<kDppRor8>((T)0, u);
  return sum_of_8_lanes(u);
}
// Two values per lane (a target's x and y terms) -> the 64-lane total of x in lanes 16-31, of y in lanes 48-63: one swap of
// halves, four DPP adds inside the rows, one row broadcast (lane 15 of rows 0 and 2 into rows 1 and 3).
constexpr int kDppRowBcast15 = 0x142;
template <class T> __device__ __forceinline__ T row_bcast15_odd_rows(T v) {  // rows 1 and 3: lane 15 of the row before; rows 0 and 2: zero
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), kDppRowBcast15, 0xa, 0xf, false));
  } else {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, kDppRowBcast15, 0xa, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), kDppRowBcast15, 0xa, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
  }
}
template <class T> __device__ __forceinline__ T reduce2(T x, T y) {
  swap_halves(x, y);
  T s = x + y;  // lanes 0-31: x.lo + x.hi, lanes 32-63: y.lo + y.hi
  s = s + dpp_of<kDppRor8>((T)0, s);
  s = sum_of_8_lanes(s);
  return s + row_bcast15_odd_rows(s);
}
template <class T> __device__ __forceinline__ T lane_fetch(T v, int src_lane) {  // v of lane src_lane (per-lane index)
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane << 2, __builtin_bit_cast(int, v)));
  } else {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(unsigned)u);
    const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
  }
}
// pair_term_fast's scale factor: term = d * scale (force 0 makes the term an exact zero: lanes past a leaf's end)
__device__ __forceinline__ float fast_scale(float dx, float dy, float force, float clamp) {
  const float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
  const float d2 = __builtin_fmaxf(__builtin_fmaf(dy, dy, dx * dx), clamp);
  return force * __builtin_amdgcn_rcpf(__builtin_fmaf(sum, d2, 8.0779356694631609e-28f));  // 2^-90
}
[[maybe_unused]] __device__ __forceinline__ double fast_scale(double dx, double dy, double force, double clamp) {
  const double sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  const double d2 = __builtin_fmax(__builtin_fma(dy, dy, dx * dx), clamp);
  const double den = __builtin_fma(sum, d2, 0x1p-700);
  double r = __builtin_amdgcn_rcp(den);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  return force * r;
}
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
[[maybe_unused]] __device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

}  // namespace nbody
