// libnbody_hip — the direct-sum driver: the kernel configuration and workspace layout of a step, the mass classes, the
// preparation / run split multi.hip shards over devices, the hipGraph replay of step pairs, and the direct entry points
// of the C ABI (nbody_update_direct_f32 / _f64, nbody_accel_direct_f32 / _f64, nbody_direct_*_dev).  The sum at points that are
// not bodies (the probe call, the tracers' share of a step) is target_driver.hip.
// Kernels: direct_kernels.hip, direct_mutual.hip, nearfar.hip, direct64.hip.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "direct64.h"
#include "direct_layout.h"
#include "driver.h"

using namespace nbody;

namespace nbody {
namespace {

// How the direct kernel covers (n_tgt x n_src): enough waves to fill 256 CUs x 4 SIMDs x 8 waves.
DirectConfig choose_direct_config(int64_t n_src, int64_t n_tgt) {
  DirectConfig c;
  c.use_asm = lab_int("NBODY_DIRECT_ASM", 4);
  // near/far split: 0.05 ms (65 536 bodies) to 0.16 ms (1 M) of preparation per step against 10 % of the pair work: it pays
  // from 65 536 x 65 536 pairs on (profiles/r03_nearfar_hash_grid.txt; the sort-based split of rounds 1-2 broke even at
  // twice that).  NBODY_DIRECT_NEARFAR: 0 never, 1 by size (default), 2 always.
  const int nf = env_int("NBODY_DIRECT_NEARFAR", 1);
  c.nearfar = nf == 2 || (nf == 1 && (double)n_src * (double)n_tgt >= 4294967296.0);
  // measured at N = 1M (profiles/r01_direct_mass_variants.txt): 1 target/thread with the hand-ordered block wins for
  // equal masses (44.0 %) and for per-body masses (39.8 % vs 36.1 % for 2 targets/thread)
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
  size_t partial = (size_t)choose_direct_config(n_src, n_tgt).gsplit * (size_t)n_tgt * sizeof(float2);
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
}  // namespace

// Flag words, partial sums, near/far scratch, and the mutual area where the pass can engage: in this order.
DirectLayout direct_layout(int64_t n_src, int64_t n_tgt_max) {
  DirectLayout L;
  L.partial = DirectLayout::flags + kFlagBytes;
  L.partial_bytes = direct_partial_bytes(n_src, n_tgt_max);
  L.nearfar = L.partial + L.partial_bytes;
  L.nf = nearfar_layout(n_src);
  L.total = L.nearfar + L.nf.total;
  if (n_tgt_max == n_src && n_src >= lab_int("NBODY_DIRECT_MUTUAL_MIN_N", (int)kMutualMinN) && n_src <= kMutualMaxN) {
    L.mutual = (L.total + 255) & ~(size_t)255;
    L.total = L.mutual + mutual_area_bytes(n_src);
  }
  return L;
}

namespace {
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
// or more runs, each over a block of targets (ctx.h: DirectStep, DirectBlock).  The plan is what both derive from the step:
// it carries the workspace layout, so they cannot disagree on it.
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
  DirectLayout L;
};
int direct_plan(nbody_ctx* c, const DirectStep& s, DirectPlan* out) {  // (checks the step's own arguments)
  if (s.n_src < 0 || s.n_tgt_total < 0 || s.n_tgt_max < 0 || s.n_tgt_max > s.n_tgt_total || s.n_tgt_total > s.n_src || s.n_src > 0x7fffffffLL)
    return fail(c, NBODY_ERR_INVALID, "direct_step: bad target/source counts");
  if (s.arith < NBODY_ARITH_AUTO || s.arith > NBODY_ARITH_EXACT) return fail(c, NBODY_ERR_INVALID, "direct_step: bad arith");
  DirectPlan p;
  p.L = direct_layout(s.n_src, s.n_tgt_max);
  if (!s.ws || s.ws_bytes < p.L.total) return fail(c, NBODY_ERR_INVALID, "direct_step: workspace too small");
  p.arith = direct_arith_f32(s.arith, s.clamp);
  p.uni = s.uniform_mass > 0.f && lab_int("NBODY_DIRECT_NO_UNIFORM", 0) == 0;
  {
    const DirectConfig c0 = choose_direct_config(s.n_src, s.n_tgt_total);
    p.nearfar = c0.nearfar;
    p.couples = c0.nearfar && c0.use_asm >= 2 && c0.tpt == 1;
  }
  // uniform_mass < 0: every mass is -uniform_mass except a sparse set; the split hands those to direct_finish, so the
  // main pass runs at the equal-mass rate.  Without the split (small problems) the per-body-mass kernel is used.
  if (s.uniform_mass < 0.f && p.nearfar && lab_int("NBODY_DIRECT_NO_UNIFORM", 0) == 0 && lab_int("NBODY_DIRECT_NO_SPARSE", 0) == 0)
    p.sparse_base = -s.uniform_mass;
  if (!p.uni && p.sparse_base == 0.f && p.nearfar) p.classes = classes_for(c, s.n_src, s.mass_all);
  p.stream_m = !p.uni && p.sparse_base == 0.f && !p.classes && p.couples && lab_int("NBODY_DIRECT_ASM", 4) >= 3;
  // lab NBODY_DIRECT_ASM: 4 (default) = mutual where it applies, else as 3
  p.mutual = p.arith != NBODY_ARITH_EXACT && p.couples && (p.uni || p.sparse_base > 0.f) && !p.classes && s.n_tgt_max == s.n_tgt_total &&
             p.L.mutual != DirectLayout::kNoMutual && lab_int("NBODY_DIRECT_ASM", 4) >= 4;
  p.use_hazard = p.arith == NBODY_ARITH_AUTO;
  *out = p;
  return NBODY_OK;
}

// The argument checks of a block, each written once.  `whole`: the block is the whole step (nbody_direct_step_dev), where a source
// count beyond int is a bad range too.
int check_range(nbody_ctx* c, const DirectStep& s, const DirectBlock& b, bool whole) {
  if (b.n_tgt < 0 || b.tgt_begin < 0 || b.tgt_begin + b.n_tgt > s.n_src || b.n_tgt > s.n_tgt_max || (whole && s.n_src > 0x7fffffffLL))
    return fail(c, NBODY_ERR_INVALID, "direct_step: bad target/source range");
  return NBODY_OK;
}
int check_arrays(nbody_ctx* c, const DirectStep& s, const DirectBlock* b) {  // b == null: the preparation, which has no outputs
  if (!s.pos_all || !s.mass_all) return fail(c, NBODY_ERR_INVALID, "direct_step: null pos_all/mass_all");
  if (b && (b->vel == nullptr) != (b->pos_out == nullptr))
    return fail(c, NBODY_ERR_INVALID, "direct_step: vel and pos_out must both be given or both be NULL");
  return !b || b->vel || b->acc_out ? NBODY_OK : fail(c, NBODY_ERR_INVALID, "direct_step: nothing to compute");
}

}  // namespace

// Decides, on the stream, which kernels of this step do the work (flags[kFlagState]).
int ctx_direct_prep(nbody_ctx* c, const DirectStep& s) {
  DirectPlan p;
  int rc = direct_plan(c, s, &p);
  if (rc || s.n_tgt_total == 0 || p.arith == NBODY_ARITH_EXACT) return rc;
  rc = check_arrays(c, s, nullptr);
  if (rc) return rc;
  int* flags = direct_flags(s.ws);
  HIPCHK(c, hipMemsetAsync(flags, 0, kFlagBytes, s.stream));
  if (p.use_hazard && !(p.nearfar && s.n_src > 0))  // (with the split on, nf_insert checks the positions as it reads them)
    HIPCHK(c, launch_hazard_scan(s.stream, (const float*)s.pos_all, 2 * s.n_src, flags));
  if (p.nearfar) {
    const float2* pos_far = nullptr;  // (where launch_nearfar says it put them: the places the layout's accessors name)
    const uint32_t* near_list = nullptr;
    const float* minv_far = nullptr;
    HIPCHK(c, launch_nearfar(s.stream, (const float2*)s.pos_all, (const float*)s.mass_all, p.sparse_base, (int)s.n_src, s.clamp, p.use_hazard,
                             flags, direct_nearfar(s.ws, p.L), p.L.nf, &pos_far, &near_list, p.classes ? p.classes->rank : nullptr,
                             p.classes ? p.classes->pad_slots : nullptr, p.classes ? p.classes->n_pad_slots : 0, p.couples,
                             p.stream_m ? &minv_far : nullptr));
  } else {
    HIPCHK(c, launch_decide_simple(s.stream, p.use_hazard, flags));
  }
  return NBODY_OK;
}

// Force + integration for the block's targets under the decision ctx_direct_prep left in the workspace.
int ctx_direct_run(nbody_ctx* c, const DirectStep& s, const DirectBlock& b) {
  int rc = check_range(c, s, b, false);
  DirectPlan p;
  if (!rc) rc = direct_plan(c, s, &p);
  if (rc || b.n_tgt == 0) return rc;
  rc = check_arrays(c, s, &b);
  if (rc) return rc;

  DirectConfig cfg = choose_direct_config(s.n_src, b.n_tgt);
  cfg.nearfar = p.nearfar;
  while (cfg.gsplit > 1 && (size_t)cfg.gsplit * (size_t)b.n_tgt * sizeof(float2) > p.L.partial_bytes) --cfg.gsplit;
  if ((size_t)cfg.gsplit * (size_t)b.n_tgt * sizeof(float2) > p.L.partial_bytes)
    return fail(c, NBODY_ERR_INVALID, "direct_step: the partial sums of this block do not fit the workspace's layout");
  DirectArgs a{};
  a.pos_all = (const float2*)s.pos_all;
  a.src_pos = a.pos_all;
  a.mass_all = (const float*)s.mass_all;
  a.n_src = (int)s.n_src;
  a.tgt_begin = (int)b.tgt_begin;
  a.n_tgt = (int)b.n_tgt;
  a.vel = (float2*)b.vel;
  a.pos_out = (float2*)b.pos_out;
  a.acc_out = (float2*)b.acc_out;
  a.partial = direct_partial(s.ws, p.L);
  a.delta = b.delta;
  a.clamp = s.clamp;
  a.uniform_mass = p.uni ? s.uniform_mass : 0.f;
  a.flags = direct_flags(s.ws);
  a.run_state = -1;

  if (p.arith == NBODY_ARITH_EXACT) {
    TimerScope ts(b.timer, s.stream);
    HIPCHK(c, launch_direct_exact(s.stream, a));
    return NBODY_OK;
  }
  const uint32_t* near_list = cfg.nearfar ? direct_near_list(s.ws, p.L) : nullptr;
  {
    TimerScope ts(b.timer, s.stream);
    if (cfg.nearfar) {  // state 0: main pass over the far sources without the clamp, near sources added by finish
      DirectArgs a0 = a;
      a0.src_pos = direct_pos_far(s.ws, p.L);
      a0.src_couples = p.couples ? 1 : 0;
      a0.src_minv = p.stream_m ? direct_minv_far(s.ws, p.L) : nullptr;
      if (p.couples) a0.n_src = (int)far_padded(s.n_src);
      a0.near_list = near_list;
      a0.to_partial = 1;
      a0.run_state = 0;
      if (p.sparse_base > 0.f) a0.uniform_mass = p.sparse_base;  // the odd masses sit in the near list (state 1 reads them all)
      if (p.classes) {  // the far copy is in class order, padded: the equal-mass instantiation, a tile's mass in its closing FMA
        a0.n_src = (int)(p.couples ? far_padded(p.classes->n_slots) : p.classes->n_slots);
        a0.uniform_mass = 1.0f;
        a0.tile_mass = p.classes->tile_mass;
      }
      if (p.mutual)  // the mutual pass and its partial reduction, both inside the timer: one far sum per target in a.partial
        HIPCHK(c, launch_direct_mutual(s.stream, a0, direct_mutual_area(s.ws, p.L, s.n_src)));
      else
        HIPCHK(c, launch_direct_fast(s.stream, a0, cfg, true));
    }
    DirectArgs a1 = a;  // state 1: one clamped pass over every source
    a1.to_partial = cfg.gsplit > 1;
    a1.run_state = 1;
    HIPCHK(c, launch_direct_fast(s.stream, a1, cfg, false));
  }
  if (cfg.nearfar) {
    DirectArgs a0 = a;
    a0.near_list = near_list;
    a0.run_state = 0;
    HIPCHK(c, launch_direct_finish(s.stream, a0, p.mutual ? 1 : cfg.gsplit, true));
  }
  if (cfg.gsplit > 1) {
    DirectArgs a1 = a;
    a1.run_state = 1;
    HIPCHK(c, launch_direct_finish(s.stream, a1, cfg.gsplit, false));
  }
  if (p.use_hazard) {  // state 2
    DirectArgs a2 = a;
    a2.run_state = 2;
    HIPCHK(c, launch_direct_exact(s.stream, a2));
  }
  return NBODY_OK;
}

namespace {
// One call for a whole step whose block is all its targets: the block's checks come first (an empty block needs no workspace).
int direct_step_dev(nbody_ctx* c, DirectStep s, const DirectBlock& b) {
  s.n_tgt_total = s.n_tgt_max = b.n_tgt;
  int rc = check_range(c, s, b, true);
  if (rc || b.n_tgt == 0) return rc;
  rc = check_arrays(c, s, &b);
  if (!rc) rc = ctx_direct_prep(c, s);
  return rc ? rc : ctx_direct_run(c, s, b);
}

DirectStep ctx_whole_step(const nbody_ctx* c, const void* pos) {  // the step of a context over all its f32 bodies, from `pos`
  const State<float>& s = c->sf;
  return DirectStep{c->stream, s.n, pos, s.set[s.cur].mass, direct_mass_hint(s), c->params.clamp, c->params.arith, s.n, s.n,
                    c->workspace, c->workspace_bytes};
}
// Everything a captured pair of steps bakes in (ctx.h: DirectGraph).
DirectGraphKey direct_graph_key(const nbody_ctx* c, float delta) {
  const State<float>& s = c->sf;
  const auto& st = s.set[s.cur];
  DirectGraphKey k;
  k.n = s.n; k.pos_a = st.pos; k.pos_b = s.pos_next; k.vel = st.vel; k.mass = st.mass; k.ws = c->workspace;
  k.delta = delta; k.clamp = c->params.clamp; k.uniform = direct_mass_hint(s); k.arith = c->params.arith;
  k.row_epoch = s.row_epoch; k.cls_usable = s.classes.usable; k.cls_rank = s.classes.rank; k.cls_tile_mass = s.classes.tile_mass;
  k.env = direct_env_signature();
  return k;
}

}  // namespace

int ctx_ensure_workspace(nbody_ctx* c, size_t bytes) { return ensure_dev_bytes(c, c->workspace, c->workspace_bytes, bytes); }
size_t ctx_direct_ws_bytes(int64_t n_src, int64_t n_tgt) { return direct_layout(n_src, n_tgt).total; }
int ctx_ensure_mass_classes(nbody_ctx* c) { return c && c->has_f32 ? ensure_mass_classes(c) : NBODY_OK; }

}  // namespace nbody

NB_API int nbody_update_direct_f32(nbody_ctx* c, float delta, int n_steps, nbody_counting* counter) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return nbody::multi_update_direct(c, delta, n_steps, counter);
  if (!c->has_f32) return fail(c, NBODY_ERR_INVALID, "update_direct_f32: no f32 particles uploaded");
  if (n_steps < 0) return fail(c, NBODY_ERR_INVALID, "update_direct_f32: n_steps < 0");
  HIPCHK(c, hipSetDevice(c->device));
  State<float>& s = c->sf;
  int rc = ctx_ensure_workspace(c, ctx_direct_ws_bytes(s.n, s.n));
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
    const DirectGraphKey key = direct_graph_key(c, delta);
    if (!g.exec || !(g.key == key)) {
      g.reset();
      hipGraph_t graph = nullptr;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
      int rc1 = NBODY_OK, rc2 = NBODY_OK;
      if (e == hipSuccess) {
        rc1 = direct_step_dev(c, ctx_whole_step(c, st.pos), DirectBlock{0, s.n, st.vel, s.pos_next, nullptr, delta, nullptr});
        if (!rc1) rc2 = direct_step_dev(c, ctx_whole_step(c, s.pos_next), DirectBlock{0, s.n, st.vel, st.pos, nullptr, delta, nullptr});
        e = hipStreamEndCapture(c->stream, &graph);
      }
      if (e == hipSuccess && !rc1 && !rc2 && graph) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
      if (e != hipSuccess || rc1 || rc2 || !g.exec) {
        g.reset();  // capture is an optimisation: fall through to eager steps
        (void)hipGetLastError();
      } else {
        g.key = key;
      }
    }
    if (g.exec) {
      for (; step + 2 <= n_steps; step += 2) HIPCHK(c, hipGraphLaunch(g.exec, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // an even number of steps: positions are back in st.pos
    }
  }
  for (; step < n_steps; ++step) {
    auto& st = s.set[s.cur];
    rc = direct_step_dev(c, ctx_whole_step(c, st.pos), DirectBlock{0, s.n, st.vel, s.pos_next, nullptr, delta, c->timer});
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
  int rc = ctx_ensure_workspace(c, ctx_direct_ws_bytes(s.n, s.n));
  if (rc) return rc;
  rc = ensure_mass_classes(c);
  if (rc) return rc;
  rc = direct_step_dev(c, ctx_whole_step(c, s.set[s.cur].pos), DirectBlock{0, s.n, nullptr, nullptr, s.acc, 0.f, c->timer});
  if (rc) return rc;
  if (s.n) HIPCHK(c, hipMemcpyAsync(acc_xy, s.acc, (size_t)s.n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

NB_API size_t nbody_direct_workspace_bytes(int64_t n_sources, int64_t n_targets) {
  if (n_sources < 0 || n_targets < 0) return 0;
  return ctx_direct_ws_bytes(n_sources, n_targets);
}

NB_API int nbody_direct_step_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all,
                                 float uniform_mass, int64_t target_begin, int64_t n_targets, void* vel, void* pos_out, void* acc_out,
                                 float delta, float clamp, int arith, void* workspace, size_t workspace_bytes,
                                 nbody_timer* timer) {
  return direct_step_dev(nullptr, DirectStep{(hipStream_t)stream, n_sources, pos_all, mass_all, uniform_mass, clamp, arith, 0, 0, workspace, workspace_bytes},
                         DirectBlock{target_begin, n_targets, vel, pos_out, acc_out, delta, timer});
}

NB_API int nbody_direct_workspace_peek(void* stream, const void* workspace, int32_t out[4]) {
  if (!workspace || !out) return fail(nullptr, NBODY_ERR_INVALID, "workspace_peek: bad arguments");
  hipError_t e = hipMemcpyAsync(out, workspace, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  return e == hipSuccess ? NBODY_OK : fail_hip(nullptr, e, "workspace_peek");
}

// The near/far split alone (launch_nearfar: no main pass, no finish) over host arrays, for tests that pin the classifier and
// what it hands its consumers.  The block is the flag words followed by the near/far scratch, every byte 0xA5 before the flag
// words are zeroed: a slot the split leaves unwritten shows.
NB_API int nbody_selftest_nearfar(int device, const float* pos_xy, const float* mass, int64_t n, float heavy_base, float clamp, int use_hazard,
                                  int couples, int with_minv, int32_t* out_flags, uint32_t* out_is_near, uint32_t* out_scan,
                                  uint32_t* out_near_list, float* out_far, float* out_minv) {
  if (!pos_xy || n < 1 || n > ((int64_t)1 << 24) || !out_flags || !out_is_near || !out_scan || !out_near_list || !out_far)
    return fail(nullptr, NBODY_ERR_INVALID, "selftest_nearfar: bad arguments");
  if ((!mass && (heavy_base > 0.f || with_minv)) || (with_minv && (!couples || !out_minv)))
    return fail(nullptr, NBODY_ERR_INVALID, "selftest_nearfar: the inverse masses need masses, couples and a place to go");
  if (hipSetDevice(device) != hipSuccess) return NBODY_ERR_NO_DEVICE;
  const NearFarLayout L = nearfar_layout(n);
  char* block = nullptr;   // flag words | near/far scratch
  float* in = nullptr;     // positions | masses
  auto finish = [&](hipError_t e) {
    (void)hipDeviceSynchronize();
    (void)hipFree(block);
    (void)hipFree(in);
    return e == hipSuccess ? NBODY_OK : fail_hip(nullptr, e, "selftest_nearfar");
  };
  hipError_t e;
  if ((e = hipMalloc((void**)&block, kFlagBytes + L.total)) != hipSuccess) return finish(e);
  if ((e = hipMalloc((void**)&in, (size_t)n * 3 * sizeof(float))) != hipSuccess) return finish(e);
  float* mass_d = mass ? in + 2 * n : nullptr;
  if ((e = hipMemcpy(in, pos_xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return finish(e);
  if (mass && (e = hipMemcpy(mass_d, mass, (size_t)n * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return finish(e);
  if ((e = hipMemset(block, 0xA5, kFlagBytes + L.total)) != hipSuccess) return finish(e);
  int* flags = (int*)block;
  char* scratch = block + kFlagBytes;
  if ((e = hipMemsetAsync(flags, 0, kFlagBytes, nullptr)) != hipSuccess) return finish(e);
  const float2* pos_far = nullptr;
  const uint32_t* near_list = nullptr;
  const float* minv_far = nullptr;
  if ((e = launch_nearfar(nullptr, (const float2*)in, mass_d, heavy_base, (int)n, clamp, use_hazard, flags, scratch, L, &pos_far, &near_list, nullptr,
                          nullptr, 0, couples != 0, with_minv ? &minv_far : nullptr)) != hipSuccess)
    return finish(e);
  if ((e = hipDeviceSynchronize()) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_flags, flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_is_near, scratch + L.is_near, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_scan, scratch + L.scan, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  const int64_t n_near = std::min<int64_t>(std::max<int64_t>(out_flags[kFlagNearCount], 0), n);
  if (n_near && (e = hipMemcpy(out_near_list, near_list, (size_t)n_near * 4, hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  const size_t far_floats = 2 * (size_t)(couples ? far_padded(n) : n);
  if ((e = hipMemcpy(out_far, pos_far, far_floats * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if (with_minv && (e = hipMemcpy(out_minv, minv_far, (size_t)far_padded(n) * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  return finish(hipSuccess);
}

NB_API int nbody_weights_to_mass_dev(void* stream, int64_t n, const void* weight_u32, void* mass_f32) {
  if (n < 0 || (n > 0 && (!weight_u32 || !mass_f32))) return fail(nullptr, NBODY_ERR_INVALID, "weights_to_mass: bad arguments");
  hipError_t e = launch_weights_to_mass((hipStream_t)stream, (const uint32_t*)weight_u32, (float*)mass_f32, n);
  return e == hipSuccess ? NBODY_OK : fail_hip(nullptr, e, "weights_to_mass");
}

NB_API int nbody_direct_prep_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all, float uniform_mass,
                                 int64_t n_targets_total, int64_t n_targets_max, float clamp, int arith, void* workspace,
                                 size_t workspace_bytes) {
  return ctx_direct_prep(nullptr, DirectStep{(hipStream_t)stream, n_sources, pos_all, mass_all, uniform_mass, clamp, arith, n_targets_total,
                                             n_targets_max, workspace, workspace_bytes});
}
NB_API int nbody_direct_run_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all, float uniform_mass,
                                int64_t target_begin, int64_t n_targets, void* vel, void* pos_out, void* acc_out, float delta,
                                float clamp, int arith, int64_t n_targets_total, int64_t n_targets_max, void* workspace,
                                size_t workspace_bytes, nbody_timer* timer) {
  return ctx_direct_run(nullptr, DirectStep{(hipStream_t)stream, n_sources, pos_all, mass_all, uniform_mass, clamp, arith, n_targets_total,
                                            n_targets_max, workspace, workspace_bytes},
                        DirectBlock{target_begin, n_targets, vel, pos_out, acc_out, delta, timer});
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
  const bool fast = direct_fast_f64(c->params.arith, a.clamp);
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
