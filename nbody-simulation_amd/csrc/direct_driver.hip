// libnbody_hip — the direct-sum driver: the kernel configuration and workspace layout of a step, the mass classes, the
// preparation / run split multi.hip shards over devices, the hipGraph replay of step pairs, and the direct entry points
// of the C ABI (nbody_update_direct_f32, nbody_accel_direct_f32, nbody_direct_*_dev), and the f64 direct entry points
// (nbody_update_direct_f64, nbody_accel_direct_f64), and the direct sum at arbitrary points (nbody_accel_direct_at_f32 / _f64),
// and the tracers' share of a direct step.
// Kernels: direct_kernels.hip, nearfar.hip, direct64.hip, direct_probe.hip, tracers.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "direct64.h"
#include "direct_kernels.h"
#include "direct_probe.h"
#include "driver.h"
#include "tracers.h"

using namespace nbody;

namespace nbody {
namespace {

// How the direct kernel covers (n_tgt x n_src): enough waves to fill 256 CUs x 4 SIMDs x 8 waves.
DirectConfig choose_direct_config(int64_t n_src, int64_t n_tgt, bool uniform = true) {
  DirectConfig c;
  c.use_asm = lab_int("NBODY_DIRECT_ASM", 4);
  // near/far split: 0.05 ms (65 536 bodies) to 0.16 ms (1 M) of preparation per step against 10 % of the pair work: it pays
  // from 65 536 x 65 536 pairs on (profiles/r03_nearfar_hash_grid.txt; the sort-based split of rounds 1-2 broke even at
  // twice that).  NBODY_DIRECT_NEARFAR: 0 never, 1 by size (default), 2 always.
  const int nf = env_int("NBODY_DIRECT_NEARFAR", 1);
  c.nearfar = nf == 2 || (nf == 1 && (double)n_src * (double)n_tgt >= 4294967296.0);
  // measured at N = 1M (profiles/r01_direct_mass_variants.txt): 1 target/thread with the hand-ordered block wins for
  // equal masses (44.0 %) and for per-body masses (39.8 % vs 36.1 % for 2 targets/thread)
  (void)uniform;
  c.tpt = lab_int("NBODY_DIRECT_TPT", 1);
  if (c.tpt != 1 && c.tpt != 2) c.tpt = 1;
  // 256 CUs x 32 wave slots hold 8192 waves; several rounds of waves balance the tail, so the sources are split
  // over blockIdx.y until there are ~16 rounds (measured, profiles/r01_direct_gsplit_sweep.txt: 131072 targets
  // 40.5 % -> 43.8 %, 65536 x 65536 33.5 % -> 43.1 %, 1M x 1M 43.8 % -> 44.1 %)
  const int64_t want_waves = 131072;
  int64_t waves = 4 * ((n_tgt + 64 * c.tpt - 1) / (64 * c.tpt));
  int64_t g = waves > 0 ? (want_waves + waves - 1) / waves : 1;
  if (g < 1) g = 1;
  if (g > 16) g = 16;
  // ... and until a split's sources (8 B each) are at most half an XCD's 4 MB L2, where 16 splits can do that: the work-groups of
  // one split run together (blockIdx.x varies fastest), so the range they stream stays L2-resident instead of being re-read
  // from HBM by waves that have drifted apart (N = 1 M: 2 -> 4 splits, FETCH_SIZE 524 -> 82 MB per launch, the same 173.1 ms)
  const int64_t g_l2 = (n_src + 262143) / 262144;
  if (g_l2 <= 16 && g < g_l2) g = g_l2;
  g = lab_int("NBODY_DIRECT_GSPLIT", (int)g);
  if (g < 1) g = 1;
  if (g > 64) g = 64;
  while (g > 1 && n_src / g < 2048) g /= 2;  // a split should still hold a couple of tiles
  c.gsplit = (int)g;
  return c;
}

constexpr size_t kFlagBytes = 256;

// The partial-sum area holds gsplit(n) x n entries for every block size n <= n_tgt (a shard's last block may be
// shorter than the others and then takes a LARGER gsplit: 262080 rows -> 9 where 262144 -> 8).  gsplit(n) =
// ceil(want_waves / (4 ceil(n/64))) <= 16, so gsplit(n) n < 2097152 + n and <= 16 n; ctx_direct_run clamps what an
// environment override could still push past it.
size_t direct_partial_bytes(int64_t n_src, int64_t n_tgt) {
  size_t partial = 0;
  for (bool uni : {false, true}) {
    DirectConfig c = choose_direct_config(n_src, n_tgt, uni);
    size_t p = (size_t)c.gsplit * (size_t)n_tgt * sizeof(float2);
    if (p > partial) partial = p;
  }
  size_t any_block = (size_t)std::min<int64_t>(16 * n_tgt, 2097152 + n_tgt) * sizeof(float2);
  if (any_block > partial) partial = any_block;
  const int64_t g_l2 = (n_src + 262143) / 262144;  // (the L2 rule of choose_direct_config holds for every block size)
  if (g_l2 <= 16 && (size_t)(g_l2 * n_tgt) * sizeof(float2) > partial) partial = (size_t)(g_l2 * n_tgt) * sizeof(float2);
  return (partial + 255) & ~(size_t)255;
}
// The mutual main pass (direct_mutual.hip) can engage when one block of targets covers every source, from its crossover on
// (measured: profiles/r06_mutual_crossover.txt) up to 2^22 bodies (beyond, the per-strip reduction's full passes over the running sums
// would pass 0.4 % of the step; untested).  Its strip buffers then follow the near/far scratch in the workspace.
constexpr int64_t kMutualMinN = 393216;
constexpr int64_t kMutualMaxN = 4194304;
bool mutual_sizes(int64_t n_src, int64_t n_tgt) {
  return n_tgt == n_src && n_src >= lab_int("NBODY_DIRECT_MUTUAL_MIN_N", (int)kMutualMinN) && n_src <= kMutualMaxN;
}
size_t mutual_offset(int64_t n_src, int64_t n_tgt) {
  return (kFlagBytes + direct_partial_bytes(n_src, n_tgt) + nearfar_layout(n_src).total + 255) & ~(size_t)255;
}
size_t direct_ws_bytes(int64_t n_src, int64_t n_tgt) {
  const size_t base = kFlagBytes + direct_partial_bytes(n_src, n_tgt) + nearfar_layout(n_src).total;
  return mutual_sizes(n_src, n_tgt) ? mutual_offset(n_src, n_tgt) + mutual_area_bytes(n_src) : base;
}

// Mass classes of the context's f32 rows in their current order (ctx.h, State::MassClasses): built on the host from the
// weights (static between uploads; only the row order moves, with the tree builds), cached until the rows are permuted.
// Classes are taken in ascending weight, bodies inside a class in ascending row: everything downstream stays a function
// of the inputs alone (bitwise reproducible).  Not used for equal masses, for "one mass but for a few bodies" (the near
// list carries those) or for more than 32 distinct masses (the per-body kernel runs then).
int ensure_mass_classes(nbody_ctx* c) {
  State<float>& s = c->sf;
  auto& mc = s.classes;
  if (mc.epoch == s.row_epoch) return NBODY_OK;
  // A captured direct step (DirectGraph) has the class arrays' addresses baked into its kernel arguments: they are about to be
  // freed and rebuilt for the new row order, so the graph goes with them (an even number of tree steps permutes the
  // rows and leaves every pointer of the graph's key where it was).
  c->direct_graph.reset();
  mc.epoch = s.row_epoch;
  mc.usable = false;
  const int64_t n = s.n;
  if (lab_int("NBODY_DIRECT_NO_CLASSES", 0) != 0 || s.uniform_mass > 0.f || s.sparse_base > 0.f || n < 32768) return NBODY_OK;
  if (s.h_weight_stale) {
    s.h_weight.resize((size_t)n);
    HIPCHK(c, hipMemcpyAsync(s.h_weight.data(), s.set[s.cur].weight, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.h_weight_stale = false;
  }
  uint32_t vals[kMaxMassClasses];
  int64_t counts[kMaxMassClasses];
  int k = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t w = s.h_weight[(size_t)i];
    int j = 0;
    while (j < k && vals[j] != w) ++j;
    if (j == k) {
      if (k == (int)kMaxMassClasses) return NBODY_OK;  // too many distinct masses
      vals[k] = w;
      counts[k] = 0;
      ++k;
    }
    ++counts[j];
  }
  if (k < 2) return NBODY_OK;
  int order[kMaxMassClasses];
  for (int j = 0; j < k; ++j) order[j] = j;
  std::sort(order, order + k, [&](int a, int b) { return vals[a] < vals[b]; });
  int64_t start[kMaxMassClasses], fill[kMaxMassClasses];
  int64_t slots = 0;
  std::vector<float> tile_mass;
  std::vector<uint32_t> pads;
  for (int r = 0; r < k; ++r) {
    const int j = order[r];
    start[j] = slots;
    fill[j] = 0;
    const int64_t padded = (counts[j] + kDirectTile - 1) / kDirectTile * kDirectTile;
    for (int64_t t = 0; t < padded / kDirectTile; ++t) tile_mass.push_back((float)vals[j]);  // `weight as f32`, main.rs:360
    for (int64_t q = slots + counts[j]; q < slots + padded; ++q) pads.push_back((uint32_t)q);
    slots += padded;
  }
  std::vector<uint32_t> rank((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t w = s.h_weight[(size_t)i];
    int j = 0;
    while (vals[j] != w) ++j;
    rank[(size_t)i] = (uint32_t)(start[j] + fill[j]++);
  }
  free_dev(mc.rank); free_dev(mc.pad_slots); free_dev(mc.tile_mass);
  HIPCHK(c, hipMalloc((void**)&mc.rank, (size_t)n * 4));
  HIPCHK(c, hipMalloc((void**)&mc.pad_slots, (pads.size() + 1) * 4));
  HIPCHK(c, hipMalloc((void**)&mc.tile_mass, (tile_mass.size() + 1) * 4));
  HIPCHK(c, hipMemcpyAsync(mc.rank, rank.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if (!pads.empty()) HIPCHK(c, hipMemcpyAsync(mc.pad_slots, pads.data(), pads.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(mc.tile_mass, tile_mass.data(), tile_mass.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  mc.n_classes = k;
  mc.n_slots = slots;
  mc.n_pad_slots = (int)pads.size();
  mc.usable = true;
  if (env_int("NBODY_TRACE", 0) != 0)
    std::fprintf(stderr, "[nbody] direct: %d mass classes, %lld bodies in %lld slots\n", k, (long long)n, (long long)slots);
  return NBODY_OK;
}
// the classes of `c` if they describe exactly these sources in their current row order
const State<float>::MassClasses* classes_for(const nbody_ctx* c, int64_t n_src, const void* mass_all) {
  if (!c || !c->has_f32) return nullptr;
  const State<float>& s = c->sf;
  const auto& mc = s.classes;
  if (!mc.usable || mc.epoch != s.row_epoch || n_src != s.n || mass_all != (const void*)s.set[s.cur].mass) return nullptr;
  return &mc;
}

// A direct step = one preparation over ALL positions (hazard scan, near/far split, the decision word) followed by one
// or more runs, each over a block of targets.  `n_tgt_total` (all targets this device computes in the step) decides
// whether the near/far split pays; `n_tgt_max` (the largest block of one run) sizes the partial-sum area, so that
// preparation and runs agree on the workspace layout.
struct DirectPlan {
  int arith = 0;
  bool uni = false;
  float sparse_base = 0.f;  // > 0: all masses equal this but a few bodies', which travel with the near list
  const State<float>::MassClasses* classes = nullptr;  // masses in a few classes: the far copy in class order, equal-mass arithmetic per tile
  bool nearfar = false;
  bool couples = false;  // the far copy in couples {xA, xB, yA, yB}, padded to whole 16-source iterations (the packed kernels)
  bool stream_m = false; // free per-body masses through the streamed main pass: the far copy carries 1 / mass in slot order
  bool mutual = false;   // the mutual main pass (direct_mutual.hip): each far pair once, equal-mass rate, one block of all targets
  int use_hazard = 0;
  size_t partial_bytes = 0;
};
int direct_plan(nbody_ctx* c, int64_t n_src, const void* mass_all, float uniform_mass, int64_t n_tgt_total, int64_t n_tgt_max, float clamp,
                int arith, const void* ws, size_t ws_bytes, DirectPlan* out) {
  if (n_src < 0 || n_tgt_total < 0 || n_tgt_max < 0 || n_tgt_max > n_tgt_total || n_tgt_total > n_src || n_src > 0x7fffffffLL)
    return fail(c, NBODY_ERR_INVALID, "direct_step: bad target/source counts");
  if (arith < NBODY_ARITH_AUTO || arith > NBODY_ARITH_EXACT) return fail(c, NBODY_ERR_INVALID, "direct_step: bad arith");
  if (!ws || ws_bytes < direct_ws_bytes(n_src, n_tgt_max)) return fail(c, NBODY_ERR_INVALID, "direct_step: workspace too small");
  // FAST's zero-distance bias needs clamp >= 2^-19 (HISTORY.md §4.1); smaller clamps always take EXACT.
  if (arith != NBODY_ARITH_EXACT && !(clamp >= 1.9073486328125e-06f)) arith = NBODY_ARITH_EXACT;
  DirectPlan p;
  p.arith = arith;
  p.uni = uniform_mass > 0.f && lab_int("NBODY_DIRECT_NO_UNIFORM", 0) == 0;
  {
    const DirectConfig c0 = choose_direct_config(n_src, n_tgt_total, p.uni);
    p.nearfar = c0.nearfar;
    p.couples = c0.nearfar && c0.use_asm >= 2 && c0.tpt == 1;
  }
  // uniform_mass < 0: every mass is -uniform_mass except a sparse set; the split hands those to direct_finish, so the
  // main pass runs at the equal-mass rate.  Without the split (small problems) the per-body-mass kernel is used.
  if (uniform_mass < 0.f && p.nearfar && lab_int("NBODY_DIRECT_NO_UNIFORM", 0) == 0 && lab_int("NBODY_DIRECT_NO_SPARSE", 0) == 0)
    p.sparse_base = -uniform_mass;
  if (!p.uni && p.sparse_base == 0.f && p.nearfar) p.classes = classes_for(c, n_src, mass_all);
  p.stream_m = !p.uni && p.sparse_base == 0.f && !p.classes && p.couples && lab_int("NBODY_DIRECT_ASM", 4) >= 3;
  // lab NBODY_DIRECT_ASM: 4 (default) = mutual where it applies, else as 3
  p.mutual = arith != NBODY_ARITH_EXACT && p.couples && (p.uni || p.sparse_base > 0.f) && !p.classes && n_tgt_max == n_tgt_total &&
             mutual_sizes(n_src, n_tgt_total) && lab_int("NBODY_DIRECT_ASM", 4) >= 4;
  p.use_hazard = arith == NBODY_ARITH_AUTO;
  p.partial_bytes = direct_partial_bytes(n_src, n_tgt_max);
  *out = p;
  return NBODY_OK;
}

}  // namespace

// Decides, on the stream, which kernels of this step do the work (flags[kFlagState]).
int ctx_direct_prep(nbody_ctx* c, hipStream_t stream, int64_t n_src, const void* pos_all, const void* mass_all, float uniform_mass,
                    int64_t n_tgt_total, int64_t n_tgt_max, float clamp, int arith, void* ws, size_t ws_bytes) {
  DirectPlan p;
  int rc = direct_plan(c, n_src, mass_all, uniform_mass, n_tgt_total, n_tgt_max, clamp, arith, ws, ws_bytes, &p);
  if (rc) return rc;
  if (n_tgt_total == 0 || p.arith == NBODY_ARITH_EXACT) return NBODY_OK;
  if (!pos_all || !mass_all) return fail(c, NBODY_ERR_INVALID, "direct_step: null pos_all/mass_all");
  int* flags = (int*)ws;
  HIPCHK(c, hipMemsetAsync(flags, 0, kFlagBytes, stream));
  if (p.use_hazard && !(p.nearfar && n_src > 0))  // (with the split on, nf_insert checks the positions as it reads them)
    HIPCHK(c, launch_hazard_scan(stream, (const float*)pos_all, 2 * n_src, flags));
  if (p.nearfar) {
    char* nf_scratch = (char*)ws + kFlagBytes + p.partial_bytes;
    NearFarLayout L = nearfar_layout(n_src);
    const float2* pos_far = nullptr;
    const uint32_t* near_list = nullptr;
    const float* minv_far = nullptr;
    HIPCHK(c, launch_nearfar(stream, (const float2*)pos_all, (const float*)mass_all, p.sparse_base, (int)n_src, clamp, p.use_hazard, flags,
                             nf_scratch, L, &pos_far, &near_list, p.classes ? p.classes->rank : nullptr,
                             p.classes ? p.classes->pad_slots : nullptr, p.classes ? p.classes->n_pad_slots : 0, p.couples,
                             p.stream_m ? &minv_far : nullptr));
  } else {
    HIPCHK(c, launch_decide_simple(stream, p.use_hazard, flags));
  }
  return NBODY_OK;
}

// Force + integration for the targets [tgt_begin, tgt_begin + n_tgt) under the decision ctx_direct_prep left in `ws`.
int ctx_direct_run(nbody_ctx* c, hipStream_t stream, int64_t n_src, const void* pos_all, const void* mass_all, float uniform_mass,
                   int64_t tgt_begin, int64_t n_tgt, void* vel, void* pos_out, void* acc_out, float delta, float clamp, int arith,
                   int64_t n_tgt_total, int64_t n_tgt_max, void* ws, size_t ws_bytes, nbody_timer* timer) {
  if (n_tgt < 0 || tgt_begin < 0 || tgt_begin + n_tgt > n_src || n_tgt > n_tgt_max)
    return fail(c, NBODY_ERR_INVALID, "direct_step: bad target/source range");
  DirectPlan p;
  int rc = direct_plan(c, n_src, mass_all, uniform_mass, n_tgt_total, n_tgt_max, clamp, arith, ws, ws_bytes, &p);
  if (rc) return rc;
  if (n_tgt == 0) return NBODY_OK;
  if (!pos_all || !mass_all) return fail(c, NBODY_ERR_INVALID, "direct_step: null pos_all/mass_all");
  if ((vel == nullptr) != (pos_out == nullptr))
    return fail(c, NBODY_ERR_INVALID, "direct_step: vel and pos_out must both be given or both be NULL");
  if (!vel && !acc_out) return fail(c, NBODY_ERR_INVALID, "direct_step: nothing to compute");

  DirectConfig cfg = choose_direct_config(n_src, n_tgt, p.uni);
  cfg.nearfar = p.nearfar;
  while (cfg.gsplit > 1 && (size_t)cfg.gsplit * (size_t)n_tgt * sizeof(float2) > p.partial_bytes) --cfg.gsplit;
  if ((size_t)cfg.gsplit * (size_t)n_tgt * sizeof(float2) > p.partial_bytes)
    return fail(c, NBODY_ERR_INVALID, "direct_step: the partial sums of this block do not fit the workspace's layout");
  int* flags = (int*)ws;
  DirectArgs a{};
  a.pos_all = (const float2*)pos_all;
  a.src_pos = a.pos_all;
  a.mass_all = (const float*)mass_all;
  a.n_src = (int)n_src;
  a.tgt_begin = (int)tgt_begin;
  a.n_tgt = (int)n_tgt;
  a.vel = (float2*)vel;
  a.pos_out = (float2*)pos_out;
  a.acc_out = (float2*)acc_out;
  a.partial = (float2*)((char*)ws + kFlagBytes);
  a.delta = delta;
  a.clamp = clamp;
  a.uniform_mass = p.uni ? uniform_mass : 0.f;
  a.flags = flags;
  a.run_state = -1;

  if (p.arith == NBODY_ARITH_EXACT) {
    TimerScope ts(timer, stream);
    HIPCHK(c, launch_direct_exact(stream, a));
    return NBODY_OK;
  }
  const float2* pos_far = nullptr;
  const uint32_t* near_list = nullptr;
  const float* minv_far = nullptr;
  if (cfg.nearfar) {
    char* nf_scratch = (char*)ws + kFlagBytes + p.partial_bytes;
    NearFarLayout L = nearfar_layout(n_src);
    pos_far = (const float2*)(nf_scratch + L.pos_far);
    near_list = (const uint32_t*)(nf_scratch + L.near_list);
    if (p.stream_m) minv_far = (const float*)(nf_scratch + L.minv_far);
  }
  {
    TimerScope ts(timer, stream);
    if (cfg.nearfar) {  // state 0: main pass over the far sources without the clamp, near sources added by finish
      DirectArgs a0 = a;
      a0.src_pos = pos_far;
      a0.src_couples = p.couples ? 1 : 0;
      a0.src_minv = minv_far;
      if (p.couples) a0.n_src = (int)far_padded(n_src);
      a0.near_list = near_list;
      a0.to_partial = 1;
      a0.run_state = 0;
      if (p.sparse_base > 0.f) a0.uniform_mass = p.sparse_base;  // the odd masses sit in the near list (state 1 reads them all)
      if (p.classes) {  // the far copy is in class order, padded: the equal-mass instantiation, a tile's mass in its closing FMA
        a0.n_src = (int)(p.couples ? far_padded(p.classes->n_slots) : p.classes->n_slots);
        a0.uniform_mass = 1.0f;
        a0.tile_mass = p.classes->tile_mass;
      }
      if (p.mutual) {  // the mutual pass and its partial reduction, both inside the timer: one far sum per target in a.partial
        char* nf_scratch = (char*)ws + kFlagBytes + p.partial_bytes;
        NearFarLayout L = nearfar_layout(n_src);
        char* area = (char*)ws + mutual_offset(n_src, n_tgt_max);
        HIPCHK(c, launch_direct_mutual(stream, a0, mutual_area(area, n_src, (const uint32_t*)(nf_scratch + L.is_near),
                                                                (const uint32_t*)(nf_scratch + L.scan))));
      } else {
        HIPCHK(c, launch_direct_fast(stream, a0, cfg, true));
      }
    }
    DirectArgs a1 = a;  // state 1: one clamped pass over every source
    a1.to_partial = cfg.gsplit > 1;
    a1.run_state = 1;
    HIPCHK(c, launch_direct_fast(stream, a1, cfg, false));
  }
  if (cfg.nearfar) {
    DirectArgs a0 = a;
    a0.near_list = near_list;
    a0.run_state = 0;
    HIPCHK(c, launch_direct_finish(stream, a0, p.mutual ? 1 : cfg.gsplit, true));
  }
  if (cfg.gsplit > 1) {
    DirectArgs a1 = a;
    a1.run_state = 1;
    HIPCHK(c, launch_direct_finish(stream, a1, cfg.gsplit, false));
  }
  if (p.use_hazard) {  // state 2
    DirectArgs a2 = a;
    a2.run_state = 2;
    HIPCHK(c, launch_direct_exact(stream, a2));
  }
  return NBODY_OK;
}

namespace {
int direct_step_dev(nbody_ctx* c, hipStream_t stream, int64_t n_src, const void* pos_all, const void* mass_all,
                    float uniform_mass, int64_t tgt_begin, int64_t n_tgt, void* vel, void* pos_out, void* acc_out,
                    float delta, float clamp, int arith, void* ws, size_t ws_bytes, nbody_timer* timer) {
  if (n_src < 0 || n_tgt < 0 || tgt_begin < 0 || tgt_begin + n_tgt > n_src || n_src > 0x7fffffffLL)
    return fail(c, NBODY_ERR_INVALID, "direct_step: bad target/source range");
  if (n_tgt == 0) return NBODY_OK;
  if (!pos_all || !mass_all) return fail(c, NBODY_ERR_INVALID, "direct_step: null pos_all/mass_all");
  if ((vel == nullptr) != (pos_out == nullptr))
    return fail(c, NBODY_ERR_INVALID, "direct_step: vel and pos_out must both be given or both be NULL");
  if (!vel && !acc_out) return fail(c, NBODY_ERR_INVALID, "direct_step: nothing to compute");
  int rc = ctx_direct_prep(c, stream, n_src, pos_all, mass_all, uniform_mass, n_tgt, n_tgt, clamp, arith, ws, ws_bytes);
  if (rc) return rc;
  return ctx_direct_run(c, stream, n_src, pos_all, mass_all, uniform_mass, tgt_begin, n_tgt, vel, pos_out, acc_out, delta, clamp, arith,
                    n_tgt, n_tgt, ws, ws_bytes, timer);
}

}  // namespace

int ctx_ensure_workspace(nbody_ctx* c, size_t bytes) { return ensure_dev_bytes(c, c->workspace, c->workspace_bytes, bytes); }
size_t ctx_direct_ws_bytes(int64_t n_src, int64_t n_tgt) { return direct_ws_bytes(n_src, n_tgt); }
int ctx_ensure_mass_classes(nbody_ctx* c) { return c && c->has_f32 ? ensure_mass_classes(c) : NBODY_OK; }

}  // namespace nbody

// ---- tracers (ctx.h, Tracers; kernels: tracers.hip and the probe call's FAST passes)
// The tracers' share of one direct step, enqueued behind the bodies' kernels of that step and before its buffers swap: `pos` /
// `mass` are the bodies at their pre-step positions, which the step's kernels only read.  Routing as nbody_accel_direct_at_*
// (below), but nothing comes back to the host: tracer_mark reads the decision word the bodies' step has just written to the
// workspace and every tracer's pre-step position, and leaves one mark per tracer (which of the two finishing kernels integrates
// it) and a decision word of the tracers' own at the head of ctx->probe_ws, which gates the f32 FAST main pass (the f64 pass has
// no gate: it runs for nothing in a step whose bodies left the f64 FAST domain).  The FAST partial sums go through ctx->probe_ws
// in batches of the probe call's size, so the workspace is bounded whatever the number of tracers.
namespace {
constexpr size_t kTracerFlagBytes = 256;

int tracer_batch(nbody_ctx* c, int64_t m, size_t elem, int64_t max_partial, int gsplit, int64_t* batch) {
  const int64_t b = std::min<int64_t>(1 << 20, max_partial / gsplit) / 256 * 256;
  *batch = std::min<int64_t>(m, std::max<int64_t>(b, 256));
  return ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, kTracerFlagBytes + (size_t)*batch * elem * (size_t)gsplit);
}

int tracers_direct_f32(nbody_ctx* c, const float2* pos, const float* mass, float delta) {
  const Tracers& tr = c->tracers;
  if (tr.m == 0) return NBODY_OK;
  const State<float>& s = c->sf;
  const int64_t n = s.n, m = tr.m;
  const float clamp = c->params.clamp;
  int arith = c->params.arith;
  if (arith != NBODY_ARITH_EXACT && !(clamp >= 1.9073486328125e-06f)) arith = NBODY_ARITH_EXACT;  // as direct_plan
  float2 *tpos = (float2*)tr.pos, *tvel = (float2*)tr.vel;
  if (arith == NBODY_ARITH_EXACT || n == 0) {
    HIPCHK(c, launch_tracer_exact<float>(c->stream, pos, mass, n, tpos, tvel, m, clamp, delta, nullptr));
    return NBODY_OK;
  }
  TracerRoute r;
  if (arith == NBODY_ARITH_AUTO) {  // the step's own decision (kFlagState == 2: a body outside FAST's domain), and the per-tracer exception
    r.word = (const int*)c->workspace;
    r.word_kind = kTracerWordState;
    r.per_target = 1;
  }
  const int g = probe_gsplit_f32(n);
  int64_t batch = 0;
  int rc = tracer_batch(c, m, sizeof(float2), (int64_t)1 << 23, g, &batch);
  if (rc) return rc;
  int* state = (int*)c->probe_ws;
  float2* part = (float2*)((char*)c->probe_ws + kTracerFlagBytes);
  HIPCHK(c, launch_tracer_mark<float>(c->stream, tpos, m, r, tr.mark, state));
  for (int64_t b0 = 0; b0 < m; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, m - b0);
    DirectArgs a{};
    a.pos_all = tpos + b0;  // the tracers ...
    a.src_pos = pos;        // ... and the bodies
    a.mass_all = mass;
    a.n_src = (int)n;
    a.tgt_begin = 0;
    a.n_tgt = (int)nb;
    a.partial = part;
    a.to_partial = 1;
    a.clamp = clamp;
    a.uniform_mass = s.uniform_mass > 0.f ? s.uniform_mass : 0.f;
    a.flags = state;
    a.run_state = 1;  // (tracer_mark wrote 2 when the step-level route is EXACT: the pass returns at once)
    DirectConfig cfg;
    cfg.tpt = 1;
    cfg.gsplit = g;
    cfg.use_asm = 2;  // the packed pass through LDS, with the clamp: the probe call's main pass
    cfg.nearfar = false;
    HIPCHK(c, launch_direct_fast(c->stream, a, cfg, false));
    HIPCHK(c, launch_tracer_finish<float>(c->stream, part, g, nb, tpos + b0, tvel + b0, delta, tr.mark + b0));
  }
  if (r.per_target) HIPCHK(c, launch_tracer_exact<float>(c->stream, pos, mass, n, tpos, tvel, m, clamp, delta, tr.mark));  // the fix-up pass
  return NBODY_OK;
}

int tracers_direct_f64(nbody_ctx* c, const double2* pos, const double* mass, double delta) {
  const Tracers& tr = c->tracers;
  if (tr.m == 0) return NBODY_OK;
  const int64_t n = c->sd.n, m = tr.m;
  const double clamp = (double)c->params.clamp;  // as direct64_step
  double2 *tpos = (double2*)tr.pos, *tvel = (double2*)tr.vel;
  if (!(c->params.arith == NBODY_ARITH_FAST && clamp > 0.0) || n == 0) {
    HIPCHK(c, launch_tracer_exact<double>(c->stream, pos, mass, n, tpos, tvel, m, clamp, delta, nullptr));
    return NBODY_OK;
  }
  TracerRoute r;
  r.word = (const int*)c->workspace;  // the domain flag the f64 step has just scanned the bodies into
  r.word_kind = kTracerWordDomain64;
  r.per_target = 1;
  const int g = probe_gsplit_f64(n);
  int64_t batch = 0;
  int rc = tracer_batch(c, m, sizeof(double2), (int64_t)1 << 22, g, &batch);
  if (rc) return rc;
  double2* part = (double2*)((char*)c->probe_ws + kTracerFlagBytes);
  HIPCHK(c, launch_tracer_mark<double>(c->stream, tpos, m, r, tr.mark, (int*)c->probe_ws));
  for (int64_t b0 = 0; b0 < m; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, m - b0);
    HIPCHK(c, launch_probe_fast_pass_f64(c->stream, pos, mass, n, tpos + b0, nb, clamp, part));
    HIPCHK(c, launch_tracer_finish<double>(c->stream, part, g, nb, tpos + b0, tvel + b0, delta, tr.mark + b0));
  }
  HIPCHK(c, launch_tracer_exact<double>(c->stream, pos, mass, n, tpos, tvel, m, clamp, delta, tr.mark));  // the fix-up pass
  return NBODY_OK;
}
}  // namespace

NB_API int nbody_update_direct_f32(nbody_ctx* c, float delta, int n_steps, nbody_counting* counter) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return nbody::multi_update_direct(c, delta, n_steps, counter);
  if (!c->has_f32) return fail(c, NBODY_ERR_INVALID, "update_direct_f32: no f32 particles uploaded");
  if (n_steps < 0) return fail(c, NBODY_ERR_INVALID, "update_direct_f32: n_steps < 0");
  HIPCHK(c, hipSetDevice(c->device));
  State<float>& s = c->sf;
  int rc = ctx_ensure_workspace(c, direct_ws_bytes(s.n, s.n));
  if (rc) return rc;
  const double t_begin = now_s();
  int step = 0;
  // ---- graph replay of step pairs (no timer attached: event records do not belong in a captured graph)
  // (nor with tracers present: their launches are not part of the captured pair; the eager steps give the same bits)
  const bool want_graph = n_steps >= 4 && s.n > 0 && s.n <= (1 << 17) && !c->timer && c->tracers.m == 0 && env_int("NBODY_DIRECT_GRAPH", 1) != 0;
  rc = ensure_mass_classes(c);  // (host work and copies: before any capture)
  if (rc) return rc;
  if (want_graph) {
    auto& st = s.set[s.cur];
    DirectGraph& g = c->direct_graph;
    const std::string sig = direct_env_signature();
    const auto& mc = s.classes;
    const bool stale = !g.exec || g.n != s.n || g.pos_a != st.pos || g.pos_b != s.pos_next || g.vel != st.vel ||
                       g.mass != st.mass || g.ws != c->workspace || g.delta != delta || g.clamp != c->params.clamp ||
                       g.uniform != direct_mass_hint(s) || g.arith != c->params.arith || g.env != sig || g.row_epoch != s.row_epoch ||
                       g.cls_usable != mc.usable || g.cls_rank != (const void*)mc.rank || g.cls_tile_mass != (const void*)mc.tile_mass;
    if (stale) {
      g.reset();
      hipGraph_t graph = nullptr;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
      int rc1 = NBODY_OK, rc2 = NBODY_OK;
      if (e == hipSuccess) {
        rc1 = direct_step_dev(c, c->stream, s.n, st.pos, st.mass, direct_mass_hint(s), 0, s.n, st.vel, s.pos_next, nullptr, delta,
                              c->params.clamp, c->params.arith, c->workspace, c->workspace_bytes, nullptr);
        if (!rc1)
          rc2 = direct_step_dev(c, c->stream, s.n, s.pos_next, st.mass, direct_mass_hint(s), 0, s.n, st.vel, st.pos, nullptr, delta,
                                c->params.clamp, c->params.arith, c->workspace, c->workspace_bytes, nullptr);
        e = hipStreamEndCapture(c->stream, &graph);
      }
      if (e == hipSuccess && !rc1 && !rc2 && graph) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
      if (e != hipSuccess || rc1 || rc2 || !g.exec) {
        g.reset();  // capture is an optimisation: fall through to eager steps
        (void)hipGetLastError();
      } else {
        g.n = s.n; g.pos_a = st.pos; g.pos_b = s.pos_next; g.vel = st.vel; g.mass = st.mass; g.ws = c->workspace;
        g.delta = delta; g.clamp = c->params.clamp; g.uniform = direct_mass_hint(s); g.arith = c->params.arith; g.env = sig;
        g.row_epoch = s.row_epoch; g.cls_usable = mc.usable; g.cls_rank = mc.rank; g.cls_tile_mass = mc.tile_mass;
      }
    }
    if (g.exec) {
      for (; step + 2 <= n_steps; step += 2) HIPCHK(c, hipGraphLaunch(g.exec, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // an even number of steps: positions are back in st.pos
    }
  }
  for (; step < n_steps; ++step) {
    auto& st = s.set[s.cur];
    rc = direct_step_dev(c, c->stream, s.n, st.pos, st.mass, direct_mass_hint(s), 0, s.n, st.vel, s.pos_next, nullptr, delta,
                         c->params.clamp, c->params.arith, c->workspace, c->workspace_bytes, c->timer);
    if (rc) return rc;
    rc = tracers_direct_f32(c, st.pos, st.mass, delta);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(st.pos, s.pos_next);
  }
  // force and integrate are one fused kernel: the whole call is booked under sum_gravity
  const double dt = now_s() - t_begin;
  c->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  s.tree_valid = false;
  c->steps_done += (uint64_t)n_steps;
  return NBODY_OK;
}

NB_API int nbody_accel_direct_f32(nbody_ctx* c, float* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  NB_VIA_PRIMARY(c, false, nbody_accel_direct_f32(p, acc_xy));
  if (!c->has_f32) return fail(c, NBODY_ERR_INVALID, "accel_direct_f32: no f32 particles uploaded");
  if (!acc_xy) return fail(c, NBODY_ERR_INVALID, "accel_direct_f32: acc_xy is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  State<float>& s = c->sf;
  int rc = ctx_ensure_workspace(c, direct_ws_bytes(s.n, s.n));
  if (rc) return rc;
  rc = ensure_mass_classes(c);
  if (rc) return rc;
  auto& st = s.set[s.cur];
  rc = direct_step_dev(c, c->stream, s.n, st.pos, st.mass, direct_mass_hint(s), 0, s.n, nullptr, nullptr, s.acc, 0.f, c->params.clamp,
                       c->params.arith, c->workspace, c->workspace_bytes, c->timer);
  if (rc) return rc;
  if (s.n) HIPCHK(c, hipMemcpyAsync(acc_xy, s.acc, (size_t)s.n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

NB_API size_t nbody_direct_workspace_bytes(int64_t n_sources, int64_t n_targets) {
  if (n_sources < 0 || n_targets < 0) return 0;
  return direct_ws_bytes(n_sources, n_targets);
}

NB_API int nbody_direct_step_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all,
                                 float uniform_mass, int64_t target_begin, int64_t n_targets, void* vel, void* pos_out, void* acc_out,
                                 float delta, float clamp, int arith, void* workspace, size_t workspace_bytes,
                                 nbody_timer* timer) {
  return direct_step_dev(nullptr, (hipStream_t)stream, n_sources, pos_all, mass_all, uniform_mass, target_begin, n_targets, vel,
                         pos_out, acc_out, delta, clamp, arith, workspace, workspace_bytes, timer);
}

NB_API int nbody_direct_workspace_peek(void* stream, const void* workspace, int32_t out[4]) {
  if (!workspace || !out) return fail(nullptr, NBODY_ERR_INVALID, "workspace_peek: bad arguments");
  hipError_t e = hipMemcpyAsync(out, workspace, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  return e == hipSuccess ? NBODY_OK : fail_hip(nullptr, e, "workspace_peek");
}

NB_API int nbody_weights_to_mass_dev(void* stream, int64_t n, const void* weight_u32, void* mass_f32) {
  if (n < 0 || (n > 0 && (!weight_u32 || !mass_f32))) return fail(nullptr, NBODY_ERR_INVALID, "weights_to_mass: bad arguments");
  hipError_t e = launch_weights_to_mass((hipStream_t)stream, (const uint32_t*)weight_u32, (float*)mass_f32, n);
  return e == hipSuccess ? NBODY_OK : fail_hip(nullptr, e, "weights_to_mass");
}

NB_API int nbody_direct_prep_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all, float uniform_mass,
                                 int64_t n_targets_total, int64_t n_targets_max, float clamp, int arith, void* workspace,
                                 size_t workspace_bytes) {
  return ctx_direct_prep(nullptr, (hipStream_t)stream, n_sources, pos_all, mass_all, uniform_mass, n_targets_total, n_targets_max, clamp,
                     arith, workspace, workspace_bytes);
}
NB_API int nbody_direct_run_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all, float uniform_mass,
                                int64_t target_begin, int64_t n_targets, void* vel, void* pos_out, void* acc_out, float delta,
                                float clamp, int arith, int64_t n_targets_total, int64_t n_targets_max, void* workspace,
                                size_t workspace_bytes, nbody_timer* timer) {
  return ctx_direct_run(nullptr, (hipStream_t)stream, n_sources, pos_all, mass_all, uniform_mass, target_begin, n_targets, vel, pos_out,
                    acc_out, delta, clamp, arith, n_targets_total, n_targets_max, workspace, workspace_bytes, timer);
}


// ---- f64: one device, EXACT unless FAST is asked for (AUTO is EXACT, as for the f64 tree walks); direct64.h
namespace {
int direct64_step(nbody_ctx* c, double delta, bool integrate) {
  State<double>& s = c->sd;
  auto& st = s.set[s.cur];
  Direct64Args a;
  a.pos = st.pos;
  a.mass = st.mass;
  a.n = s.n;
  if (integrate) {
    a.vel = st.vel;
    a.pos_out = s.pos_next;
  } else {
    a.acc_out = s.acc;
  }
  a.delta = delta;
  a.clamp = (double)c->params.clamp;  // the f32 parameter widened, as the oracle's np.float32(clamp) -> T
  const bool fast = c->params.arith == NBODY_ARITH_FAST && a.clamp > 0.0;  // (a NaN clamp fails the test too)
  TimerScope ts(c->timer, c->stream);
  HIPCHK(c, launch_direct64(c->stream, a, fast, c->workspace, c->workspace_bytes));
  return NBODY_OK;
}
}  // namespace

NB_API int nbody_update_direct_f64(nbody_ctx* c, double delta, int n_steps, nbody_counting* counter) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return fail(c, NBODY_ERR_INVALID, "update_direct_f64: multi-device direct steps are f32 only");
  if (!c->has_f64) return fail(c, NBODY_ERR_INVALID, "update_direct_f64: no f64 particles uploaded");
  if (n_steps < 0) return fail(c, NBODY_ERR_INVALID, "update_direct_f64: n_steps < 0");
  HIPCHK(c, hipSetDevice(c->device));
  State<double>& s = c->sd;
  int rc = ctx_ensure_workspace(c, direct64_ws_bytes(s.n));
  if (rc) return rc;
  const double t_begin = now_s();
  for (int step = 0; step < n_steps && (s.n > 0 || c->tracers.m > 0); ++step) {
    rc = s.n > 0 ? direct64_step(c, delta, true) : NBODY_OK;
    if (rc) return rc;
    rc = tracers_direct_f64(c, s.set[s.cur].pos, s.set[s.cur].mass, delta);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(s.set[s.cur].pos, s.pos_next);
  }
  // force and integrate are one fused kernel: the whole call is booked under sum_gravity
  const double dt = now_s() - t_begin;
  c->counting.sum_gravity += dt;
  if (counter) counter->sum_gravity += dt;
  s.tree_valid = false;
  c->steps_done += (uint64_t)n_steps;
  return NBODY_OK;
}

NB_API int nbody_accel_direct_f64(nbody_ctx* c, double* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return fail(c, NBODY_ERR_INVALID, "accel_direct_f64: multi-device direct steps are f32 only");
  if (!c->has_f64) return fail(c, NBODY_ERR_INVALID, "accel_direct_f64: no f64 particles uploaded");
  if (!acc_xy) return fail(c, NBODY_ERR_INVALID, "accel_direct_f64: acc_xy is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  State<double>& s = c->sd;
  int rc = ctx_ensure_workspace(c, direct64_ws_bytes(s.n));
  if (rc) return rc;
  if (s.n == 0) return NBODY_OK;
  rc = direct64_step(c, 0.0, false);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(acc_xy, s.acc, (size_t)s.n * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}


// ---- the direct sum at arbitrary points (nbody_accel_direct_at_*; kernels: direct_probe.hip, and the step's clamped FAST pass)
// Routing, per call, from the bodies and the params alone; per target, from its own coordinates alone (include/nbody_hip.h):
//   f32  EXACT, or a clamp below 2^-19, or AUTO with a body outside FAST's domain (what makes the step run direct_exact):
//        every target EXACT.  Otherwise FAST — under AUTO a target outside FAST's domain takes its EXACT value.
//   f64  EXACT unless FAST is asked for with a clamp > 0 and every body inside the f64 FAST domain; then FAST, a target
//        outside that domain EXACT.
// FAST f32 is the clamped packed pass of the step (direct_fast<1, *, false, 2>) over the bodies in row order, its source split
// fixed by the number of bodies (probe_gsplit_f32); the clamp is in every pair, so no near/far decision depends on the targets.
// Targets go through in batches: the workspace (ctx->probe_ws) is bounded whatever n_targets is.
namespace {

constexpr size_t kProbeFlagBytes = 256;

bool fast_domain_f32(float x, float y) {
  for (float v : {x, y}) {
    const float a = std::fabs(v);
    if (!(a < kFastBig) || (a != 0.f && a < kFastTiny)) return false;
  }
  return true;
}
bool fast_domain_f64(double x, double y) {
  for (double v : {x, y}) {
    const double a = std::fabs(v);
    if (!(a < 0x1p100) || (a != 0.0 && a < 0x1p-300)) return false;
  }
  return true;
}

// The workspace of a call once its route is known: the flag word, a batch of targets and of results, and — FAST only (`gsplit`
// > 0) — the batch's partial sums.  A batch holds at most 2^20 targets, and its partial sums at most `max_partial` entries (2^23
// f32, 2^22 f64).  *batch receives the batch size.
int probe_workspace(nbody_ctx* c, int64_t n_targets, size_t elem, int64_t max_partial, int gsplit, int64_t* batch) {
  const int64_t b = std::min<int64_t>(1 << 20, max_partial / std::max(gsplit, 1)) / 256 * 256;
  *batch = std::min<int64_t>(n_targets, std::max<int64_t>(b, 256));
  const size_t need = kProbeFlagBytes + (size_t)*batch * elem * (2 + (size_t)std::max(gsplit, 0));
  return ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, need);
}

// The device flag word of a body scan, read back: 0 all inside the domain.
int read_flag(nbody_ctx* c, const int* flag_dev, int* out) {
  HIPCHK(c, hipMemcpyAsync(out, flag_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

// Runs `pass(d_tgt, n, d_out, d_partial)` over the targets `idx` (all of them when idx is null) batch by batch and scatters the
// results into acc.
template <class T2, class Pass>
int probe_batches(nbody_ctx* c, int64_t m, const T2* tgt, const std::vector<int64_t>* idx, T2* acc, int64_t batch, Pass pass) {
  char* ws = (char*)c->probe_ws;
  T2* d_tgt = (T2*)(ws + kProbeFlagBytes);
  T2* d_out = d_tgt + batch;
  T2* d_part = d_out + batch;
  std::vector<T2> gather, result;
  const int64_t total = idx ? (int64_t)idx->size() : m;
  for (int64_t b0 = 0; b0 < total; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, total - b0);
    const T2* src = tgt + b0;
    T2* dst = acc + b0;
    if (idx) {
      gather.resize((size_t)nb);
      result.resize((size_t)nb);
      for (int64_t k = 0; k < nb; ++k) gather[(size_t)k] = tgt[(*idx)[(size_t)(b0 + k)]];
      src = gather.data();
      dst = result.data();
    }
    HIPCHK(c, hipMemcpyAsync(d_tgt, src, (size_t)nb * sizeof(T2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, pass(d_tgt, nb, d_out, d_part));
    HIPCHK(c, hipMemcpyAsync(dst, d_out, (size_t)nb * sizeof(T2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (idx)
      for (int64_t k = 0; k < nb; ++k) acc[(*idx)[(size_t)(b0 + k)]] = result[(size_t)k];
  }
  return NBODY_OK;
}

int accel_at_f32(nbody_ctx* c, int64_t m, const float2* tgt, float2* acc) {
  State<float>& s = c->sf;
  const int64_t n = s.n;
  if (n == 0) {
    std::fill(acc, acc + m, make_float2(0.f, 0.f));
    return NBODY_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const float clamp = c->params.clamp;
  int arith = c->params.arith;
  if (arith != NBODY_ARITH_EXACT && !(clamp >= 1.9073486328125e-06f)) arith = NBODY_ARITH_EXACT;  // as direct_plan
  const int g = probe_gsplit_f32(n);
  auto& st = s.set[s.cur];
  int rc = NBODY_OK;
  if (arith == NBODY_ARITH_AUTO) {  // the step's hazard scan over the bodies
    rc = ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, kProbeFlagBytes);
    if (rc) return rc;
    int* flag = (int*)c->probe_ws;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_hazard_scan(c->stream, (const float*)st.pos, 2 * n, flag));
    int bad = 0;
    rc = read_flag(c, flag, &bad);
    if (rc) return rc;
    if (bad) arith = NBODY_ARITH_EXACT;
  }
  int64_t batch = 0;
  rc = probe_workspace(c, m, sizeof(float2), (int64_t)1 << 23, arith == NBODY_ARITH_EXACT ? 0 : g, &batch);
  if (rc) return rc;
  int* flag = (int*)c->probe_ws;
  auto exact = [&](const float2* d_tgt, int64_t nb, float2* d_out, float2*) {
    return launch_probe_exact_f32(c->stream, st.pos, st.mass, n, d_tgt, nb, clamp, d_out);
  };
  if (arith == NBODY_ARITH_EXACT) return probe_batches(c, m, tgt, nullptr, acc, batch, exact);
  auto fast = [&](const float2* d_tgt, int64_t nb, float2* d_out, float2* d_part) {
    DirectArgs a{};
    a.pos_all = d_tgt;  // the targets ...
    a.src_pos = st.pos;  // ... and the bodies
    a.mass_all = st.mass;
    a.n_src = (int)n;
    a.tgt_begin = 0;
    a.n_tgt = (int)nb;
    a.partial = d_part;
    a.to_partial = 1;
    a.clamp = clamp;
    a.uniform_mass = s.uniform_mass > 0.f ? s.uniform_mass : 0.f;
    a.flags = flag;
    a.run_state = -1;
    DirectConfig cfg;
    cfg.tpt = 1;
    cfg.gsplit = g;
    cfg.use_asm = 2;  // the packed pass through LDS, with the clamp
    cfg.nearfar = false;
    hipError_t e = launch_direct_fast(c->stream, a, cfg, false);
    return e == hipSuccess ? launch_probe_finish_f32(c->stream, d_part, g, nb, d_out) : e;
  };
  rc = probe_batches(c, m, tgt, nullptr, acc, batch, fast);
  if (rc || arith != NBODY_ARITH_AUTO) return rc;
  std::vector<int64_t> odd;  // AUTO: the targets outside FAST's domain take their EXACT values
  for (int64_t i = 0; i < m; ++i)
    if (!fast_domain_f32(tgt[i].x, tgt[i].y)) odd.push_back(i);
  return odd.empty() ? NBODY_OK : probe_batches(c, m, tgt, &odd, acc, batch, exact);
}

int accel_at_f64(nbody_ctx* c, int64_t m, const double2* tgt, double2* acc) {
  State<double>& s = c->sd;
  const int64_t n = s.n;
  if (n == 0) {
    std::fill(acc, acc + m, double2{0.0, 0.0});
    return NBODY_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const double clamp = (double)c->params.clamp;  // the f32 parameter widened, as direct64_step
  bool fast = c->params.arith == NBODY_ARITH_FAST && clamp > 0.0;
  auto& st = s.set[s.cur];
  int rc = NBODY_OK;
  if (fast) {  // the f64 step's domain scan over the bodies
    rc = ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, kProbeFlagBytes);
    if (rc) return rc;
    int* flag = (int*)c->probe_ws;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_probe_domain_f64(c->stream, (const double*)st.pos, 2 * n, flag));
    int bad = 0;
    rc = read_flag(c, flag, &bad);
    if (rc) return rc;
    if (bad) fast = false;
  }
  int64_t batch = 0;
  rc = probe_workspace(c, m, sizeof(double2), (int64_t)1 << 22, fast ? probe_gsplit_f64(n) : 0, &batch);
  if (rc) return rc;
  auto pass = [&](bool f) {
    return [&, f](const double2* d_tgt, int64_t nb, double2* d_out, double2* d_part) {
      return launch_probe_f64(c->stream, st.pos, st.mass, n, d_tgt, nb, clamp, f, d_part, d_out);
    };
  };
  rc = probe_batches(c, m, tgt, nullptr, acc, batch, pass(fast));
  if (rc || !fast) return rc;
  std::vector<int64_t> odd;
  for (int64_t i = 0; i < m; ++i)
    if (!fast_domain_f64(tgt[i].x, tgt[i].y)) odd.push_back(i);
  return odd.empty() ? NBODY_OK : probe_batches(c, m, tgt, &odd, acc, batch, pass(false));
}

int accel_at_check(nbody_ctx* c, bool f64, int64_t m, const void* tgt, const void* acc) {
  const char* what = f64 ? "accel_direct_at_f64" : "accel_direct_at_f32";
  if (m < 0) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": n_targets < 0");
  if (m > 0 && (!tgt || !acc)) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": target_xy or acc_xy is NULL");
  if (f64 ? !c->has_f64 : !c->has_f32)
    return fail(c, NBODY_ERR_INVALID, std::string(what) + ((f64 ? c->has_f32 : c->has_f64)
                                                               ? ": the context holds particles of the other precision"
                                                               : ": no particles uploaded"));
  return NBODY_OK;
}

}  // namespace

namespace nbody {
int ctx_accel_direct_at(nbody_ctx* c, bool f64, int64_t n_targets, const void* target_xy, void* acc_xy) {
  if (n_targets == 0) return NBODY_OK;
  return f64 ? accel_at_f64(c, n_targets, (const double2*)target_xy, (double2*)acc_xy)
             : accel_at_f32(c, n_targets, (const float2*)target_xy, (float2*)acc_xy);
}
}  // namespace nbody

NB_API int nbody_accel_direct_at_f32(nbody_ctx* c, int64_t n_targets, const float* target_xy, float* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  int rc = accel_at_check(c, false, n_targets, target_xy, acc_xy);
  if (rc || n_targets == 0) return rc;
  if (c->multi) return multi_accel_direct_at(c, false, n_targets, target_xy, acc_xy);
  return ctx_accel_direct_at(c, false, n_targets, target_xy, acc_xy);
}
NB_API int nbody_accel_direct_at_f64(nbody_ctx* c, int64_t n_targets, const double* target_xy, double* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  int rc = accel_at_check(c, true, n_targets, target_xy, acc_xy);
  if (rc || n_targets == 0) return rc;
  if (c->multi) return multi_accel_direct_at(c, true, n_targets, target_xy, acc_xy);
  return ctx_accel_direct_at(c, true, n_targets, target_xy, acc_xy);
}
