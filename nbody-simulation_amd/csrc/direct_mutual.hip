// The mutual main pass of the direct step (gfx950): every unordered far pair evaluated ONCE (Newton's third law).
//
// For equal masses the term source j adds to target i and the one i adds to j are the same d * rcp(den) with opposite sign
// (d = p_j - p_i, den = (|dx| + |dy|) r^2 + 2^-90: direct_kernels.hip's FAST pair without the mass, which the equal-mass pass
// hoists).  The differences, squares, |dx| + |dy|, the denominator and the two reciprocals — 10 of the 12 issue slots of a
// couple in direct_stream — then serve four accumulations instead of two, for two more v_pk_fma: 14 slots per 4 ordered pairs.
//
// Work: the far copy (nearfar.hip, couples {xA, xB, yA, yB}, near bodies replaced by far markers that contribute
// exactly 0 both ways) is cut into slices of kMutualSlice slots.  A work-group of 8 waves holds one slice as targets in registers,
// 16 per lane, and takes one source slice as 64 chunks of 128 sources: lane l holds one source couple and its four
// accumulators, and after every step the couple moves one lane on (v_mov_b32_dpp wave_ror:1, 8 moves per 16 evaluations), so in
// 64 steps it meets every target of the wave.  Items are the slice pairs (s, b) with s < b, each unordered pair once, and the
// diagonal items (s, s), whose unordered pairs are also taken once (mutual_schedule.h: the wave blocks' pairs in five phases, half
// an item's steps).  A unit of work — one work-group — is an off-diagonal item or two diagonal items; the units run in strips of
// whole rounds (one launch each, at most kMutualStripItems units), whose partials live in a fixed-size area of the caller's
// workspace.  At 2^20 bodies: 8128 + 64 units, 32 rounds of 256.  No atomics, fixed orders throughout:
//   - target side: per chunk in registers, added to a running total per target (two-level summation), one partial per item;
//   - source side: off the diagonal summed over the eight waves through LDS in wave order, one partial per (item, source); on the
//     diagonal gathered in LDS in phase order and added to the target side, one partial per (diagonal, body);
//   - after each strip, direct_mutual_reduce adds the strip's partials of every body to its running sum in a.partial in a fixed
//     order (its column, its row, its diagonal); direct_finish then adds the near sources and integrates, unchanged.
// Near bodies as TARGETS (their slot holds a marker) get the far sources from direct_mutual_near, one-sided, in source ranges.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as fmaf() or in asm.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "direct_kernels.h"
#include "mutual_schedule.h"

namespace nbody {

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int kWaves = 8;                          // waves per work-group: 2 per SIMD (the body's registers: ~210 VGPRs)

constexpr int kSlice = kMutualSlice;               // = 64 lanes x 16 targets x 8 waves
constexpr int kSliceCouples = kSlice / 2;
constexpr int kChunks = kSliceCouples / 64;        // 128-source chunks per source slice
constexpr float kMarker = 1e30f;                   // nearfar.hip's far-away point

__device__ __forceinline__ bool gate_open(const DirectArgs& a) { return a.run_state < 0 || a.flags[kFlagState] == a.run_state; }

__device__ __forceinline__ float4 couple_or_marker(const float4* c, int64_t k, int64_t n_couples) {
  return k < n_couples ? c[k] : make_float4(kMarker, kMarker, kMarker, kMarker);
}

// One step: 16 (target, source couple) evaluations, two halves of 8, then the rotation.  Evaluation t = 2k + h pairs target
// couple k's half h with the lane's source couple (RX, RY):
//   DX = RX - tx, DY = RY - ty (op_sel picks the target's half for both lanes of the packed op); Q = DX DX + DY DY;
//   S = |DX| + |DY| (plain adds, issued at wave priority 0 so that two waves' adds share a slot, as in direct_stream);
//   S = S Q + 2^-90; S = 1 / S; target: AX += DX S, AY += DY S; source: SAX -= DX S, SAY -= DY S.
// Temporaries of evaluation t % 8 in v[192 + 8 (t % 8) ...]: DX +0, DY +2, Q +4, S +6.
// Wait states (nothing inside an asm string is padded by the compiler):
//   - v_rcp (trans) -> its first non-trans consumer needs 1: the reciprocals of evaluation t + 1 issue between those of t and
//     t's four FMAs;
//   - VALU write -> DPP read of the same VGPR needs 2: the ring's four moves come first (their last VALU write is a step old),
//     then SAX / SAY, at least 5 instructions after the last FMA that wrote them.
#define NB_PX(K, H, D) "v_pk_add_f32 v[" D "], v[184:185], %[tx" #K "] op_sel:[0," #H "] op_sel_hi:[1," #H "] neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define NB_PY(K, H, D) "v_pk_add_f32 v[" D "], v[186:187], %[ty" #K "] op_sel:[0," #H "] op_sel_hi:[1," #H "] neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define NB_SQ(DX, DY, Q) "v_pk_mul_f32 v[" Q "], v[" DX "], v[" DX "]\n\tv_pk_fma_f32 v[" Q "], v[" DY "], v[" DY "], v[" Q "]\n\t"
#define NB_AD(XL, XH, YL, YH, SL, SH) "v_add_f32_e64 v" SL ", |v" XL "|, |v" YL "|\n\tv_add_f32_e64 v" SH ", |v" XH "|, |v" YH "|\n\t"
#define NB_DN(S, Q) "v_pk_fma_f32 v[" S "], v[" S "], v[" Q "], %[b]\n\t"
#define NB_RC(SL, SH) "v_rcp_f32_e32 v" SL ", v" SL "\n\tv_rcp_f32_e32 v" SH ", v" SH "\n\t"
#define NB_AC(T, DX, DY, S)                                                                                                          \
  "v_pk_fma_f32 %[ax" #T "], v[" DX "], v[" S "], %[ax" #T "]\n\t"                                                                    \
  "v_pk_fma_f32 v[188:189], v[" DX "], v[" S "], v[188:189] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"                                                  \
  "v_pk_fma_f32 %[ay" #T "], v[" DY "], v[" S "], %[ay" #T "]\n\t"                                                                    \
  "v_pk_fma_f32 v[190:191], v[" DY "], v[" S "], v[190:191] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
// half Q of the step: evaluations 8Q .. 8Q + 7, target couples 4Q .. 4Q + 3
#define NB_HALF(K0, K1, K2, K3, T0, T1, T2, T3, T4, T5, T6, T7)                                                                    \
  NB_PX(K0, 0, "192:193") NB_PX(K0, 1, "200:201") NB_PX(K1, 0, "208:209") NB_PX(K1, 1, "216:217")                                   \
  NB_PX(K2, 0, "224:225") NB_PX(K2, 1, "232:233") NB_PX(K3, 0, "240:241") NB_PX(K3, 1, "248:249")                                   \
  NB_PY(K0, 0, "194:195") NB_PY(K0, 1, "202:203") NB_PY(K1, 0, "210:211") NB_PY(K1, 1, "218:219")                                   \
  NB_PY(K2, 0, "226:227") NB_PY(K2, 1, "234:235") NB_PY(K3, 0, "242:243") NB_PY(K3, 1, "250:251")                                   \
  NB_SQ("192:193", "194:195", "196:197") NB_SQ("200:201", "202:203", "204:205") NB_SQ("208:209", "210:211", "212:213")             \
  NB_SQ("216:217", "218:219", "220:221") NB_SQ("224:225", "226:227", "228:229") NB_SQ("232:233", "234:235", "236:237")             \
  NB_SQ("240:241", "242:243", "244:245") NB_SQ("248:249", "250:251", "252:253")                                                    \
  "s_setprio 0\n\t"                                                                                                                \
  NB_AD("192", "193", "194", "195", "198", "199") NB_AD("200", "201", "202", "203", "206", "207")                                  \
  NB_AD("208", "209", "210", "211", "214", "215") NB_AD("216", "217", "218", "219", "222", "223")                                  \
  NB_AD("224", "225", "226", "227", "230", "231") NB_AD("232", "233", "234", "235", "238", "239")                                  \
  NB_AD("240", "241", "242", "243", "246", "247") NB_AD("248", "249", "250", "251", "254", "255")                                  \
  "s_setprio 1\n\t"                                                                                                                \
  NB_DN("198:199", "196:197") NB_DN("206:207", "204:205") NB_DN("214:215", "212:213") NB_DN("222:223", "220:221")                 \
  NB_DN("230:231", "228:229") NB_DN("238:239", "236:237") NB_DN("246:247", "244:245") NB_DN("254:255", "252:253")                 \
  NB_RC("198", "199")                                                                                                              \
  NB_RC("206", "207") NB_AC(T0, "192:193", "194:195", "198:199")                                                                   \
  NB_RC("214", "215") NB_AC(T1, "200:201", "202:203", "206:207")                                                                   \
  NB_RC("222", "223") NB_AC(T2, "208:209", "210:211", "214:215")                                                                   \
  NB_RC("230", "231") NB_AC(T3, "216:217", "218:219", "222:223")                                                                   \
  NB_RC("238", "239") NB_AC(T4, "224:225", "226:227", "230:231")                                                                   \
  NB_RC("246", "247") NB_AC(T5, "232:233", "234:235", "238:239")                                                                   \
  NB_RC("254", "255") NB_AC(T6, "240:241", "242:243", "246:247")                                                                   \
  NB_AC(T7, "248:249", "250:251", "254:255")
#define NB_ROT(R) "v_mov_b32_dpp " R ", " R " wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"

// `steps` (>= 1) steps of a chunk: the lane's source couple rc goes into v[184:187] (RX, RY), its accumulators sacc into
// v[188:191] (SAX, SAY); both come out moved `steps` lanes up (after 64 steps every couple is back in its lane).
__device__ __forceinline__ void mutual_steps(const v2f* tx, const v2f* ty, v2f* ax, v2f* ay, float4& rc, float4& sacc, int steps,
                                             unsigned long long bias2) {
  asm volatile("v_mov_b32 v184, %[r0]\n\tv_mov_b32 v185, %[r1]\n\tv_mov_b32 v186, %[r2]\n\tv_mov_b32 v187, %[r3]\n\t"
               "v_mov_b32 v188, %[o0]\n\tv_mov_b32 v189, %[o1]\n\tv_mov_b32 v190, %[o2]\n\tv_mov_b32 v191, %[o3]\n\t"
               "s_mov_b32 s88, %[n]\n"
               ".Lnb_mutual_%=:\n\t"
               NB_HALF(0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7) NB_HALF(4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
               NB_ROT("v184") NB_ROT("v185") NB_ROT("v186") NB_ROT("v187") NB_ROT("v188") NB_ROT("v189") NB_ROT("v190") NB_ROT("v191")
               "s_sub_u32 s88, s88, 1\n\t"
               "s_cmp_lg_u32 s88, 0\n\t"
               "s_cbranch_scc1 .Lnb_mutual_%=\n\t"
               "v_mov_b32 %[o0], v188\n\tv_mov_b32 %[o1], v189\n\tv_mov_b32 %[o2], v190\n\tv_mov_b32 %[o3], v191\n\t"
               "v_mov_b32 %[r0], v184\n\tv_mov_b32 %[r1], v185\n\tv_mov_b32 %[r2], v186\n\tv_mov_b32 %[r3], v187\n\t"
               : [ax0] "+v"(ax[0]), [ax1] "+v"(ax[1]), [ax2] "+v"(ax[2]), [ax3] "+v"(ax[3]), [ax4] "+v"(ax[4]), [ax5] "+v"(ax[5]),
                 [ax6] "+v"(ax[6]), [ax7] "+v"(ax[7]), [ax8] "+v"(ax[8]), [ax9] "+v"(ax[9]), [ax10] "+v"(ax[10]), [ax11] "+v"(ax[11]),
                 [ax12] "+v"(ax[12]), [ax13] "+v"(ax[13]), [ax14] "+v"(ax[14]), [ax15] "+v"(ax[15]),
                 [ay0] "+v"(ay[0]), [ay1] "+v"(ay[1]), [ay2] "+v"(ay[2]), [ay3] "+v"(ay[3]), [ay4] "+v"(ay[4]), [ay5] "+v"(ay[5]),
                 [ay6] "+v"(ay[6]), [ay7] "+v"(ay[7]), [ay8] "+v"(ay[8]), [ay9] "+v"(ay[9]), [ay10] "+v"(ay[10]), [ay11] "+v"(ay[11]),
                 [ay12] "+v"(ay[12]), [ay13] "+v"(ay[13]), [ay14] "+v"(ay[14]), [ay15] "+v"(ay[15]),
                 [o0] "+v"(sacc.x), [o1] "+v"(sacc.y), [o2] "+v"(sacc.z), [o3] "+v"(sacc.w),
                 [r0] "+v"(rc.x), [r1] "+v"(rc.y), [r2] "+v"(rc.z), [r3] "+v"(rc.w)
               : [tx0] "v"(tx[0]), [tx1] "v"(tx[1]), [tx2] "v"(tx[2]), [tx3] "v"(tx[3]), [tx4] "v"(tx[4]), [tx5] "v"(tx[5]),
                 [tx6] "v"(tx[6]), [tx7] "v"(tx[7]), [ty0] "v"(ty[0]), [ty1] "v"(ty[1]), [ty2] "v"(ty[2]), [ty3] "v"(ty[3]),
                 [ty4] "v"(ty[4]), [ty5] "v"(ty[5]), [ty6] "v"(ty[6]), [ty7] "v"(ty[7]), [b] "s"(bias2), [n] "s"(steps)
               : "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191",
                 "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205",
                 "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219",
                 "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233",
                 "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247",
                 "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255", "s88", "scc");
}
#undef NB_PX
#undef NB_PY
#undef NB_SQ
#undef NB_AD
#undef NB_DN
#undef NB_RC
#undef NB_AC
#undef NB_HALF
#undef NB_ROT

__device__ __forceinline__ void load_targets(const float4* couples, int64_t n_couples, int s, int w, int lane, v2f* tx, v2f* ty) {
  // couples s * kSliceCouples + 512 w + 8 lane + k, k < 8 -> local slots 1024 w + 16 lane + 2 k + h
  const int64_t tc0 = (int64_t)s * kSliceCouples + 512 * w + 8 * lane;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 c = couple_or_marker(couples, tc0 + k, n_couples);
    tx[k] = v2f{c.x, c.y};
    ty[k] = v2f{c.z, c.w};
  }
}

__device__ __forceinline__ void zero_acc(v2f* ax, v2f* ay) {
#pragma unroll
  for (int t = 0; t < 16; ++t) ax[t] = ay[t] = v2f{0.f, 0.f};
}

__device__ __forceinline__ void add_chunk(const v2f* ax, const v2f* ay, float* tot_x, float* tot_y) {
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    tot_x[t] += ax[t].x + ax[t].y;
    tot_y[t] += ay[t].x + ay[t].y;
  }
}

constexpr unsigned long long kBias2 = 0x1280000012800000ull;  // {2^-90, 2^-90}

// Off-diagonal item (s, b): slice s as targets, slice b as 64 source chunks; target partials to tpart, source partials to spart.
__device__ __forceinline__ void off_item(const float4* couples, int64_t n_couples, int s, int b, int w, int lane, float4 (*red)[kWaves][64],
                                         float2* tpart, float2* spart_f2) {
  v2f tx[8], ty[8];
  load_targets(couples, n_couples, s, w, lane, tx, ty);
  float tot_x[16], tot_y[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) tot_x[t] = tot_y[t] = 0.f;
  float* spart = reinterpret_cast<float*>(spart_f2);
  for (int c = 0; c < kChunks; ++c) {
    float4 rc = couple_or_marker(couples, (int64_t)b * kSliceCouples + 64 * c + lane, n_couples);
    v2f ax[16], ay[16];
    zero_acc(ax, ay);
    float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
    mutual_steps(tx, ty, ax, ay, rc, sacc, 64, kBias2);
    add_chunk(ax, ay, tot_x, tot_y);
    // after 64 steps every couple is back in its lane; the waves' source sums meet in LDS, added in wave order
    red[c & 1][w][lane] = sacc;
    __syncthreads();  // (one barrier per chunk: buffer c & 1 is rewritten at chunk c + 2, after everyone has passed chunk c + 1's)
    if (threadIdx.x < 256) {
      const int q = threadIdx.x >> 2, comp = threadIdx.x & 3;
      float r = 0.f;
#pragma unroll
      for (int v = 0; v < kWaves; ++v) r += reinterpret_cast<const float*>(&red[c & 1][v][q])[comp];
      // source slot 128 c + 2 q + (comp & 1) of slice b, component comp >> 1 (x, y)
      spart[(size_t)(128 * c + 2 * q + (comp & 1)) * 2 + (comp >> 1)] = r;
    }
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) tpart[1024 * w + 16 * lane + t] = make_float2(tot_x[t], tot_y[t]);
}

// Diagonal item of slice s: each unordered pair of the slice once (mutual_schedule.h), the whole sum of every body to out.  The
// source sums of block u's chunk j gather in src[u][j][lane]: phase 0 writes them, phases 1 .. 4 add in phase order, one wave per
// block and phase, a barrier between phases.  A body's sum is then its target side plus its source sums.
__device__ __forceinline__ void diag_item(const float4* couples, int64_t n_couples, int s, int w, int lane, float4 (*src)[8][64],
                                          float2* out) {
  using namespace mutual_schedule;
  v2f tx[8], ty[8];
  load_targets(couples, n_couples, s, w, lane, tx, ty);
  float tot_x[16], tot_y[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) tot_x[t] = tot_y[t] = 0.f;
  const int64_t c0 = (int64_t)s * kSliceCouples;
  for (int p = 0; p < kDiagPhases; ++p) {
    const int u = diag_block(w, p), r0 = diag_first_step(w, p), n = diag_steps(p);
    for (int j = 0; j < 8; ++j) {
      // lane l loads the couple of lane l - r0 (mod 64): its first step pairs it at distance r0
      float4 rc = couple_or_marker(couples, c0 + 512 * u + 8 * ((lane - r0) & 63) + j, n_couples);
      v2f ax[16], ay[16];
      zero_acc(ax, ay);
      float4 sacc = make_float4(0.f, 0.f, 0.f, 0.f);
      int moved;
      if (p == 0) {  // diag_one_sided: steps 0 and n - 1 count for the targets only, their source terms are dropped
        mutual_steps(tx, ty, ax, ay, rc, sacc, 1, kBias2);
        sacc = make_float4(0.f, 0.f, 0.f, 0.f);
        mutual_steps(tx, ty, ax, ay, rc, sacc, n - 2, kBias2);
        const float4 keep = sacc;
        mutual_steps(tx, ty, ax, ay, rc, sacc, 1, kBias2);
        sacc = keep;
        moved = n - 1;
      } else {
        mutual_steps(tx, ty, ax, ay, rc, sacc, n, kBias2);
        moved = n;
      }
      add_chunk(ax, ay, tot_x, tot_y);
      // couple l was loaded by lane l + r0 and has moved `moved` lanes up since: its accumulators sit in lane l + r0 + moved
      const int shift = (r0 + moved) & 63;
      if (shift) {
        const int from = (lane + shift) & 63;
        sacc = make_float4(__shfl(sacc.x, from), __shfl(sacc.y, from), __shfl(sacc.z, from), __shfl(sacc.w, from));
      }
      float4& d = src[u][j][lane];
      if (p == 0) {
        d = sacc;
      } else {
        const float4 o = d;
        d = make_float4(o.x + sacc.x, o.y + sacc.y, o.z + sacc.z, o.w + sacc.w);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 q = src[w][k][lane];
    out[1024 * w + 16 * lane + 2 * k] = make_float2(tot_x[2 * k] + q.x, tot_y[2 * k] + q.z);
    out[1024 * w + 16 * lane + 2 * k + 1] = make_float2(tot_x[2 * k + 1] + q.y, tot_y[2 * k + 1] + q.w);
  }
  __syncthreads();  // (src is rewritten by the next diagonal's phase 0)
}

// Units [lo, lo + gridDim.x) of one strip; unit lo + k writes its partials to strip slot k: an off-diagonal item (s, b) its
// target partials to tpart and its source partials to spart, a diagonal unit slice s's sums to tpart and slice s + 1's to spart.
__global__ __launch_bounds__(kWaves * 64) void direct_mutual(const DirectArgs a, MutualArea m, int64_t lo) {
  if (!gate_open(a)) return;
  const int nb = m.n_slices;
  int s, b;
  mutual_schedule::unit_slices(lo + blockIdx.x, nb, s, b);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const float4* couples = reinterpret_cast<const float4*>(a.src_pos);
  const int64_t n_couples = a.n_src / 2;
  float2* tpart = m.tpart + (size_t)blockIdx.x * kSlice;
  float2* spart = m.spart + (size_t)blockIdx.x * kSlice;
  __shared__ float4 lds[8][8][64];  // off-diagonal: the source sums' exchange, [2][kWaves][64]; diagonal: the source sums
  __builtin_amdgcn_s_setprio(1);
  if (s < b) {
    off_item(couples, n_couples, s, b, w, lane, reinterpret_cast<float4(*)[kWaves][64]>(&lds[0][0][0]), tpart, spart);
  } else {
    diag_item(couples, n_couples, s, w, lane, lds, tpart);
    if (s + 1 < nb) diag_item(couples, n_couples, s + 1, w, lane, lds, spart);
  }
}

// The far sources of every NEAR body (its slot in the far copy holds a marker, so the mutual pass gave it nothing), one-sided,
// the equal-mass FAST pair without the clamp.  Block (g, y) takes the g-th of kNearSplit source ranges for near bodies y, y +
// gridDim.y, ...: its 256 threads stride the range and sum in a fixed tree; the ranges' sums go to near_part[k][g] and
// direct_mutual_reduce adds them in range order.
__global__ __launch_bounds__(256) void direct_mutual_near(const DirectArgs a, MutualArea m) {
  if (!gate_open(a)) return;
  const int n_near = a.flags[kFlagNearCount];
  const float4* couples = reinterpret_cast<const float4*>(a.src_pos);
  const int n_couples = a.n_src / 2;
  const int per = (n_couples + kMutualNearSplit - 1) / kMutualNearSplit;
  const int q0 = blockIdx.x * per, q1 = q0 + per < n_couples ? q0 + per : n_couples;
  __shared__ float2 red[256];
  for (int k = blockIdx.y; k < n_near; k += gridDim.y) {
    const float2 p = a.pos_all[a.near_list[k]];
    float ax = 0.f, ay = 0.f;
#pragma unroll 4
    for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
      const float4 c = couples[q];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float dx = (h ? c.y : c.x) - p.x, dy = (h ? c.w : c.z) - p.y;
        const float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
        const float d2 = __builtin_fmaf(dy, dy, dx * dx);
        const float s = __builtin_amdgcn_rcpf(__builtin_fmaf(sum, d2, 8.0779356694631609e-28f));
        ax = __builtin_fmaf(dx, s, ax);
        ay = __builtin_fmaf(dy, s, ay);
      }
    }
    red[threadIdx.x] = make_float2(ax, ay);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) {
        red[threadIdx.x].x += red[threadIdx.x + w].x;
        red[threadIdx.x].y += red[threadIdx.x + w].y;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) m.near_part[(size_t)k * kMutualNearSplit + blockIdx.x] = red[0];
    __syncthreads();
  }
}

// Adds strip [lo, hi)'s partials of body i to its running far sum in a.partial, in a fixed order: the source partials of its
// column (items (r, s), ascending r), the target partials of its row (items (s, b), ascending b), its diagonal.  The first
// strip starts the sum, the last multiplies it by the mass; a near body's sum comes from direct_mutual_near instead (its slot
// holds a marker: every partial of it is 0).
__global__ __launch_bounds__(256) void direct_mutual_reduce(const DirectArgs a, MutualArea m, int64_t lo, int64_t hi, int first, int last) {
  using mutual_schedule::item_of;
  if (!gate_open(a)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_tgt) return;
  const int nb = m.n_slices;
  const int s = i / kSlice, l = i % kSlice;
  // column: item_of(r, s) grows with r; the r of the strip, [r0, r1), by bisection
  int r0 = 0, r1 = s;
  while (r0 < r1) {
    const int mid = (r0 + r1) >> 1;
    if (item_of(mid, s, nb) < lo) r0 = mid + 1; else r1 = mid;
  }
  int re = s;
  r1 = r0;
  while (r1 < re) {
    const int mid = (r1 + re) >> 1;
    if (item_of(mid, s, nb) < hi) r1 = mid + 1; else re = mid;
  }
  // row: items item_of(s, s + 1) .. item_of(s, nb - 1), contiguous
  const int64_t b0 = s + 1 < nb ? item_of(s, s + 1, nb) : 0, b1 = s + 1 < nb ? item_of(s, nb - 1, nb) + 1 : 0;
  const int64_t w0 = b0 > lo ? b0 : lo, w1 = b1 < hi ? b1 : hi;
  const int64_t d = mutual_schedule::diag_unit(s, nb);
  const bool has_d = d >= lo && d < hi;
  if (r0 == r1 && w0 >= w1 && !has_d && !first && !last) return;
  float2 acc = first ? make_float2(0.f, 0.f) : a.partial[i];
#pragma unroll 8
  for (int r = r0; r < r1; ++r) {
    const float2 p = m.spart[(size_t)(item_of(r, s, nb) - lo) * kSlice + l];
    acc.x += p.x;
    acc.y += p.y;
  }
#pragma unroll 8
  for (int64_t it = w0; it < w1; ++it) {
    const float2 p = m.tpart[(size_t)(it - lo) * kSlice + l];
    acc.x += p.x;
    acc.y += p.y;
  }
  if (has_d) {
    const float2 p = ((s & 1) ? m.spart : m.tpart)[(size_t)(d - lo) * kSlice + l];
    acc.x += p.x;
    acc.y += p.y;
  }
  if (last) {
    if (m.is_near[i]) {
      const float2* np = m.near_part + (size_t)m.near_scan[i] * kMutualNearSplit;
      acc = np[0];
      for (int g = 1; g < kMutualNearSplit; ++g) {
        acc.x += np[g].x;
        acc.y += np[g].y;
      }
    }
    acc = make_float2(acc.x * a.uniform_mass, acc.y * a.uniform_mass);
  }
  a.partial[i] = acc;
}

}  // namespace

int mutual_slices(int64_t n_slots) { return (int)((n_slots + kSlice - 1) / kSlice); }

// The strip buffers (kMutualStripItems units' target and source partials: 32 MiB whatever the size of the problem) and the near
// bodies' range sums (kMutualNearSplit per near body, at most n / 64 near bodies: 4 n bytes).
size_t mutual_area_bytes(int64_t n_src) {
  return 2 * (size_t)kMutualStripItems * kSlice * sizeof(float2) + ((size_t)n_src / 64 + 2) * kMutualNearSplit * sizeof(float2);
}

MutualArea mutual_area(void* base, int64_t n_src, const uint32_t* is_near, const uint32_t* near_scan) {
  MutualArea m{};
  m.n_slices = mutual_slices(far_padded(n_src));
  float2* p = (float2*)base;
  m.tpart = p;
  p += (size_t)kMutualStripItems * kSlice;
  m.spart = p;
  p += (size_t)kMutualStripItems * kSlice;
  m.near_part = p;
  m.is_near = is_near;
  m.near_scan = near_scan;
  return m;
}

// The near bodies' far sums first, then strip by strip: the units of the strip, then their partials added to every body's sum.
// A strip is as many whole rounds of one work-group per CU as the strip area holds (mutual_schedule::strip_units).
hipError_t launch_direct_mutual(hipStream_t s, const DirectArgs& a, const MutualArea& m) {
  if (a.n_tgt <= 0) return hipSuccess;
  if (!a.src_couples || a.tgt_begin != 0 || a.n_src < a.n_tgt || m.n_slices != mutual_slices(a.n_src)) return hipErrorInvalidValue;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  if (cus <= 0) return hipErrorInvalidValue;
  const int64_t units = mutual_schedule::units(m.n_slices);
  const int64_t strip = mutual_schedule::strip_units(cus, kMutualStripItems);
  const dim3 rgrid((unsigned)((a.n_tgt + 255) / 256));
  hipLaunchKernelGGL(direct_mutual_near, dim3(kMutualNearSplit, kMutualNearRows), dim3(256), 0, s, a, m);
  for (int64_t lo = 0; lo < units; lo += strip) {
    const int64_t hi = lo + strip < units ? lo + strip : units;
    hipLaunchKernelGGL(direct_mutual, dim3((unsigned)(hi - lo)), dim3(kWaves * 64), 0, s, a, m, lo);
    hipLaunchKernelGGL(direct_mutual_reduce, rgrid, dim3(256), 0, s, a, m, lo, hi, lo == 0 ? 1 : 0, hi == units ? 1 : 0);
  }
  return hipGetLastError();
}

}  // namespace nbody
