// libnbody_hip — the Barnes-Hut step driver: the walk phase (main.rs:406-416) and its routes, the f32 BVH step enqueued whole
// ahead of the host (bvh_step_ahead), the plain and the sharded step, the row exchange of a sharded step, and the tree entry
// points of the C ABI (nbody_update_tree_*, nbody_wait, nbody_accel_tree_*, ...).  Builds: tree_build_driver.hip; phase timing: phase_clock.h.
// Kernels: walk_prepare.hip, walk_tile.hip, walk_tile_fast.hip, walk_lab.hip (launched through walk_launch.hip), tree_kernels.hip, bvh_build.hip and its units (bvh_units.h).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "bvh_build.h"
#include "driver.h"
#include "phase_clock.h"
#include "walk_split.h"

namespace nbody {

// The one-pass walk's estimate from the last walk's per-particle counts `hist` (summing to `total`): scaled down by `*shift` so
// that the scan of its total fits 31 bits.  Laboratory test hook NBODY_WALK_TILE_POISON: a history whose scan wraps, which must
// be noticed.
int estimate_shift(nbody_ctx* c, unsigned long long total, uint32_t* hist, int64_t n, int* shift) {
  int k = 0;
  while ((total >> k) >= (1ull << 31)) ++k;
  *shift = k;
  if (lab_int("NBODY_WALK_TILE_POISON", 0) != 0) HIPCHK(c, hipMemsetAsync(hist, 0xFF, (size_t)n * 4, c->stream));
  return NBODY_OK;
}

namespace {

// NBODY_WALK_SPLIT (big-leaf BVH walk): 0 the fused walk only, 1 one pass through LDS when it pays (default), 3 one pass whenever
// possible; the laboratory build also knows 4 / 2, the three-pass design of round 1 (when it pays / whenever possible).
int walk_split_mode() {
  const int mode = env_int("NBODY_WALK_SPLIT", 1);
  return (!kLabBuild && (mode == 2 || mode == 4)) ? 1 : mode;
}

// NBODY_TRACE: one line per launched walk that says WHICH walk it was.  Nearly every route computes the same bits by design,
// so the result cannot tell them apart: tests that name a route read it here (tests/_routes.py).
//   route: fused | small-leaves | per-thread (laboratory) | tile | three-pass (laboratory) | none
//   tile only: arm exact | fast-registers | fast-rows (laboratory also fast-bfs, fast-registers-log); rows, srec, rec_mode:
//   the kernel's template parameters (-1: that arm has none)
//   prep: how a tile walk's estimate was prepared: plain (library scan, wrap check, total), scan-tail (a step enqueued
//   ahead: walk_scan_est_tail) or check-tail (a step enqueued ahead: library scan + walk_check_est_tail); ahead: 0 / 1
void trace_route(const char* route, const TileRoute* t, const char* prep, bool ahead, int64_t n_tgt, bool f64) {
  if (env_int("NBODY_TRACE", 0) == 0) return;
  const TileRoute none;
  if (!t) t = &none;
  std::fprintf(stderr, "[nbody] walk route: route=%s arm=%s rows=%d srec=%d rec_mode=%d prep=%s ahead=%d n_tgt=%lld f64=%d\n", route, t->arm,
               t->rows, t->srec, t->rec_mode, prep, ahead ? 1 : 0, (long long)n_tgt, f64 ? 1 : 0);
}

// A walk in which the average target takes a sixteenth of all particles (small theta on the needle boxes) is nearly the
// direct sum: every lane wants every leaf and the fused walk's lane = target is the cheaper arrangement.
inline bool walk_near_direct(unsigned long long total, int64_t n_tgt, int64_t n) {
  return (double)total > (double)n_tgt * (double)n / 16.0;
}

// The split walks' scratch for `L`: a new one starts the estimate scan's books at zero and holds no earlier walk's counts.
template <class T> int ensure_walk_scratch(nbody_ctx* c, State<T>& s, const WalkSplitLayout& L) {
  if (s.ws_scratch_bytes >= L.total) return NBODY_OK;
  s.wt_hist_n = -1;
  int rc = ensure_dev_bytes(c, s.ws_scratch, s.ws_scratch_bytes, L.total);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(s.ws_scratch + L.scan_state, 0, L.scan_state_bytes, c->stream));  // walk_scan_est_tail keeps its books there
  return NBODY_OK;
}

// Big leaves, one pass: a leaf's terms are evaluated lane = particle and handed over through LDS (walk_tile.hip,
// walk_tile_fast.hip), the waves cut by an estimate of each target's work: the last walk's counts when these targets have a
// history, a counting traversal otherwise, none if that estimate's scan does not fit.
template <class T> int walk_one_pass(nbody_ctx* c, State<T>& s, const WalkArgs<T>& w, const WalkTargets<T>& t, const WalkOpts& o, int mode) {
  const WalkSplitLayout L = walk_split_layout(w.n_tgt);
  int rc = ensure_walk_scratch(c, s, L);
  if (rc) return rc;
  const bool self = t.ids != nullptr;
  if (self && !s.wt_hist) {
    HIPCHK(c, hipMalloc((void**)&s.wt_hist, (size_t)(s.n > 0 ? s.n : 1) * 4));
    HIPCHK(c, hipMemsetAsync(s.wt_hist, 0, (size_t)(s.n > 0 ? s.n : 1) * 4, c->stream));  // a shard's slice never writes the other ids
    s.wt_hist_n = -1;
  }
  const bool hist = self && s.wt_hist_n == w.n_tgt && s.wt_hist_begin == t.first && lab_int("NBODY_WALK_TILE_COUNT", 0) == 0;
  int shift = 0;
  if (hist && (rc = estimate_shift(c, s.wt_total, s.wt_hist, s.n, &shift)) != NBODY_OK) return rc;
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long total = 0;
  TileRoute tile_route;
  for (int estimate = hist ? 1 : 0;; estimate = 2) {
    {
      TimerScope ts(o.timer, c->stream);
      HIPCHK(c, launch_tree_walk_tile(c->stream, w, s.ws_scratch, L, t.ids, self ? s.wt_hist : nullptr, estimate, shift, &tile_route));
    }
    HIPCHK(c, hipMemcpyAsync(info, s.ws_scratch + L.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(&total, &info[6], 8);
    if (env_int("NBODY_TRACE", 0) != 0)
      std::fprintf(stderr, "[nbody] tile walk: %llu terms, estimate %s (shift %d, total %d), %d per wave, overflow %d\n", total,
                   estimate == 1 ? "from the last walk" : (estimate == 0 ? "counted" : "none"), shift, info[0], info[3], info[1]);
    trace_route("tile", &tile_route, "plain", false, w.n_tgt, sizeof(T) == 8);
    // an estimate whose scan does not fit (a counted one past 2^32 terms; counts of older walks under another theta
    // in a shard's new slice): walk without one (the counts it leaves behind are scaled next time)
    if (info[1] == 0) break;
    if (estimate == 2) return fail(c, NBODY_ERR_HIP, "tile walk: overflow flag without an estimate");
  }
  s.wt_hist_n = self ? w.n_tgt : -1;
  s.wt_hist_begin = t.first;
  s.wt_total = total;
  if (mode != 3 && walk_near_direct(total, w.n_tgt, s.n)) *o.backoff = 64;  // the fused walk; look again in 64 walks
  return NBODY_OK;
}

#ifdef NBODY_LAB
// Laboratory: three passes through a term array (walk_lab.hip; the round-1 design the one-pass walk replaced).  `*done` stays
// false when the fused walk has to do it: too many terms for this tree, or no room for them.
int walk_three_pass(nbody_ctx* c, State<float>& s, const WalkArgs<float>& w, const WalkOpts& o, bool* done) {
  s.wt_hist_n = -1;
  const int64_t hard_cap = ((int64_t)1 << 31) - 65536;  // terms (16 GB; the offsets are 32 bits wide); past that the fused walk
  const WalkSplitLayout L = walk_split_layout(w.n_tgt);
  if (int rc = ensure_walk_scratch(c, s, L)) return rc;
  for (int attempt = 0; attempt < 2 && !*done; ++attempt) {
    int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    {
      TimerScope ts(o.timer, c->stream);
      HIPCHK(c, launch_tree_walk_split(c->stream, w, s.ws_scratch, L, s.ws_terms, s.ws_capacity));
    }
    HIPCHK(c, hipMemcpyAsync(info, s.ws_scratch + L.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (env_int("NBODY_TRACE", 0) != 0)
      std::fprintf(stderr, "[nbody] split walk: %d terms, overflow %d, %d terms per term-pass wave; longest such wave %d us (leaf %d us, node %d us; timing builds)\n",
                   info[0], info[1], info[3], info[5] >> 20, (info[5] >> 10) & 1023, info[5] & 1023);
    trace_route("three-pass", nullptr, "none", false, w.n_tgt, false);
    if (info[1] == 0) {
      *done = true;
    } else if (info[2] != 0 || info[0] > hard_cap) {
      *o.backoff = 64;  // too many terms for this tree: fused walk for a while
      break;
    } else {  // the term array was too small (or absent): half as much again, once
      free_dev(s.ws_terms);
      s.ws_capacity = 0;
      int64_t want = (int64_t)info[0] + info[0] / 2 + 4096;
      if (want > hard_cap) want = hard_cap;
      if (hipMalloc(&s.ws_terms, (size_t)want * sizeof(float2)) != hipSuccess) {  // no room: the fused walk needs none
        (void)hipGetLastError();
        s.ws_terms = nullptr;
        *o.backoff = 64;
        break;
      }
      s.ws_capacity = want;
    }
  }
  return NBODY_OK;
}
#endif

// The fused walk (lane = target; tree_kernels.hip): small leaves, walks with statistics, and whatever the split walks leave.
template <class T> int walk_fused(nbody_ctx* c, const WalkArgs<T>& w, const WalkOpts& o) {
  const char* route = "none";
  {
    TimerScope ts(o.timer, c->stream);
    HIPCHK(c, launch_tree_walk<T>(c->stream, w, lab_int("NBODY_WALK_PER_THREAD", 0) == 0, &route));
  }
  trace_route(route, nullptr, "none", false, w.n_tgt, sizeof(T) == 8);
  return NBODY_OK;
}

// Phase 2 (main.rs:406-416): the installed tree walked at `t`, the accelerations to `acc`, by one of the three routes above.
// NBODY_WALK_SPLIT: 0 never a split walk, 1 one pass when it pays (default), 3 one pass whenever possible; laboratory build only:
// 4 / 2 three passes when it pays / whenever possible (the product treats them as 1).
template <class T> int tree_walk_phase(nbody_ctx* c, State<T>& s, int kind, const WalkTargets<T>& t, void* acc, const WalkOpts& o) {
  WalkArgs<T> w = walk_args(c, s, kind);
  w.n_nodes = s.n_nodes;
  w.stats = o.stats ? c->stats_dev : nullptr;
  if (w.stats) HIPCHK(c, hipMemsetAsync(c->stats_dev, 0, 3 * sizeof(unsigned long long), c->stream));
  const auto& leaves = s.set[kind == NBODY_TREE_BVH ? s.cur : 1 - s.cur];  // the quad tree's leaves own copies of their points
  w.leaf_pos = leaves.pos; w.leaf_mass = leaves.mass;
  w.tgt_pos = t.pos; w.n_tgt = t.n; w.tgt_index = t.index;
  w.acc = (typename State<T>::T2*)acc + t.acc_first;
  const int mode = walk_split_mode();
  const bool pays = w.n_tgt >= 4096 && *o.backoff == 0;
  const bool eligible = w.big_leaves && !w.stats && w.n_tgt > 0 && w.n_nodes > 0 && lab_int("NBODY_WALK_PER_THREAD", 0) == 0;
  constexpr bool lab_f32 = kLabBuild && std::is_same<T, float>::value;
  bool done = false;
  int rc = NBODY_OK;
  if (eligible && (mode == 3 || (mode == 1 && pays))) {
    rc = walk_one_pass<T>(c, s, w, t, o, mode);
    done = true;
  } else if (lab_f32 && eligible && (mode == 2 || (mode == 4 && pays))) {
    if constexpr (lab_f32) rc = walk_three_pass(c, s, w, o, &done);
  } else if (*o.backoff > 0 && eligible) {
    --*o.backoff;
  }
  if (!rc && !done) rc = walk_fused<T>(c, w, o);
  if (!rc && w.stats) HIPCHK(c, hipMemcpyAsync(c->last_stats, c->stats_dev, sizeof(c->last_stats), hipMemcpyDeviceToHost, c->stream));
  return rc;
}

// A whole f32 BVH step enqueued AHEAD of the host's knowledge of it.  The plain sequence asks the device three questions per step
// (is the build complete?  did the walk's estimate wrap?  how many terms were there?) and the old step driver added a wait at
// every phase boundary: five round trips on a 1.2 ms step.  Here the stream gets, in one go,
//     build (blind: the levels the last tree had, plus one) -> verdict of the build, ON THE DEVICE -> row gather ->
//     the walk's preparation (estimate scan, wrap check, budget) -> a 0.5 KB copy of {verdict, flags, level counters,
//     walk info} to pinned memory (StepAheadRecord) + an event -> the walk kernel, reading the node count from device memory
//     and returning at once if the verdict or the preparation said no
// and the host waits for that EVENT only — it fires when the long kernel starts, so the integration and the whole next step's
// build are enqueued while the walk runs and the stream never drains between steps.  Everything the host decides on is known
// before the walk; the rows a step starts from stay intact until it has decided (the gather writes the other set, the integration
// is enqueued after the decision), so a step whose speculation fails is simply done again by the plain sequence.  The walk's
// exact term count (next estimate's scale) is read one step late.
template <class T> int step_ahead_collect(nbody_ctx* c, State<T>& s) {  // the previous ahead-step's term count, if one is due
  if (!s.ahead_total_due) return NBODY_OK;
  s.ahead_total_due = false;
  unsigned long long total = 0;
  std::memcpy(&total, &c->spec_host->info_after[6], 8);
  s.wt_total = total;
  if (walk_near_direct(total, s.n, s.n)) s.ws_backoff = 64;  // the fused walk for a while
  return NBODY_OK;
}

struct AheadStep {  // one such step, from "it applies" to its decision
  BvhBuildLayout L;
  WalkSplitLayout WL;
  bool fused_scan = false;  // the walk's preparation is the one fused kernel (walk_scan_est_tail)
  bool stamps = false;      // the phases are timed by the step's own kernels
  StepClock clock;
  int lv_end = 0, shift = 0;  // blind levels of the build, scale of the walk's estimate
  TileRoute route;
};

// Does the step ahead apply?  NBODY_OK, or 1: take the plain sequence.  Changes nothing but what it allocates the first time.
int step_ahead_applies(nbody_ctx* c, const State<float>& s, AheadStep& a) {
  const int n = (int)s.n, leaf = c->params.leaf_size;
  if (n < 4096 || leaf < 16 || walk_split_mode() != 1 || c->want_stats || s.ws_backoff != 0) return 1;
  if (!s.wt_hist || s.wt_hist_n != n || s.wt_hist_begin != 0) return 1;  // no walk of these targets to estimate from yet
  if (env_int("NBODY_STEP_AHEAD", 1) == 0 || env_int("NBODY_TREE_BUILD_HOST", 0) != 0 || lab_int("NBODY_WALK_PER_THREAD", 0) != 0 ||
      lab_int("NBODY_WALK_TILE_COUNT", 0) != 0)
    return 1;
  a.L = bvh_build_layout(n, leaf);
  a.WL = walk_split_layout(n);
  if (s.bb_scratch_bytes < a.L.total || s.ws_scratch_bytes < a.WL.total || s.node_cap < (size_t)a.L.node_cap || s.node_aux_cap < (size_t)a.L.node_cap)
    return 1;  // the plain sequence sizes the buffers the first time
  if (a.L.bigcount - a.L.flags + kBvhLevels * sizeof(int) > sizeof(StepAheadRecord::build)) return 1;
  if (!c->spec_dev) {
    HIPCHK(c, hipMalloc((void**)&c->spec_dev, 2 * sizeof(int) + sizeof(StepAheadRecord)));
    HIPCHK(c, hipHostMalloc((void**)&c->spec_host, sizeof(StepAheadRecord), hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer((void**)&c->spec_host_dev, c->spec_host, 0));
    HIPCHK(c, hipEventCreateWithFlags(&c->spec_event, hipEventDisableTiming));
  }
  // Phase timing: by the step's own kernels when the walk's preparation is the one fused kernel; by events otherwise.
  // (one kernel instead of three: 17 us against 32 at 151 405 targets, 31 against 67 at a million; NBODY_WALK_FUSED_SCAN_MAX=0: the three)
  a.fused_scan = n <= std::min<int64_t>(kWalkFusedScanMaxTargets, lab_int("NBODY_WALK_FUSED_SCAN_MAX", (int)kWalkFusedScanMaxTargets));
  a.stamps = a.fused_scan && lab_int("NBODY_PHASE_STAMPS", 1) != 0;
  return NBODY_OK;
}

// Build, the walk's preparation, the event the host waits for, the walk: everything up to the step's one decision.
int step_ahead_enqueue(nbody_ctx* c, State<float>& s, AheadStep& a, PhaseEvents* chain) {
  const int n = (int)s.n;
  int rc = a.clock.begin(c, a.stamps, chain);
  if (rc) return rc;
  const auto &in = s.set[s.cur], &out = s.set[1 - s.cur];
  // ---- build
  a.lv_end = bvh_blind_levels(n, s.bvh_levels_hint, s.bvh_levels_stable);
  const bool flags_clean = s.bb_flags_clean;
  s.bb_flags_clean = false;
  HIPCHK(c, bvh_build_begin(c->stream, in.pos, n, s.bb_scratch, a.L, flags_clean, a.clock.stamp(0), a.clock.stamp_prev_end()));
  if (a.lv_end > 0) HIPCHK(c, bvh_build_levels(c->stream, n, c->params.leaf_size, 0, a.lv_end, s.bb_scratch, a.L));
  int* walk_info = (int*)(s.ws_scratch + a.WL.info);  // the estimate check's counters: cleared by the numbering's launch
  if ((rc = bvh_finish_gather(c, s, a.L, 0, walk_info)) || (rc = a.clock.mark(1))) return rc;
  // ---- walk (rows as after the build: `out` is the permuted set, `in` the snapshot)
  WalkArgs<float> w = walk_args(c, s, NBODY_TREE_BVH);  // (leaf >= 16: big leaves)
  const WalkTargets<float> t = self_targets(s, 1 - s.cur, NBODY_TREE_BVH, c->params.order);
  w.n_nodes = 0; w.n_nodes_dev = c->spec_dev;  // (the verdict's node count, read on the device)
  w.leaf_pos = out.pos; w.leaf_mass = out.mass;
  w.tgt_pos = t.pos; w.n_tgt = t.n; w.acc = s.acc;
  if ((rc = estimate_shift(c, s.wt_total, s.wt_hist, s.n, &a.shift)) != NBODY_OK) return rc;
  // The estimate check's last work-group concludes on the build (the verdict the walk kernel reads), packs verdict, build
  // flags and walk info for the host and clears the build's counters for the next step.
  TileTail tail;
  tail.flags = (const int*)(s.bb_scratch + a.L.flags); tail.flag_words = kAheadBuildWords;
  tail.bigcount = (const int*)(s.bb_scratch + a.L.bigcount); tail.level_end = a.lv_end; tail.node_cap = a.L.node_cap;
  tail.verdict = c->spec_dev;
  tail.pack = c->spec_host_dev->verdict;  // (straight into the host's pinned record, from its first word on: no copy on the stream)
  tail.clear = (int*)(s.bb_scratch + a.L.flags); tail.clear_words = (int)((a.L.zero_end - a.L.flags) / sizeof(int));
  tail.info_zeroed = true; tail.fused_scan = a.fused_scan; tail.stamp = a.clock.stamp(1);
  int64_t waves = 0;
  HIPCHK(c, launch_tree_walk_tile_prep<float>(c->stream, w, s.ws_scratch, a.WL, t.ids, s.wt_hist, 1, a.shift, &waves, &tail));
  s.bb_flags_clean = true;
  HIPCHK(c, hipEventRecord(c->spec_event, c->stream));  // (the tail kernel has written the record up to info_before by then)
  {
    TimerScope ts(c->timer, c->stream);
    HIPCHK(c, launch_tree_walk_tile_main<float>(c->stream, w, s.ws_scratch, a.WL, t.ids, s.wt_hist, waves, &a.route));
  }
  return a.clock.mark(2);
}

// The step's one wait — for the event in front of the walk kernel — and what follows from the record: 1 (nothing was integrated,
// the rows are intact: the plain sequence does the step), or the build stands and the step is integrated.
int step_ahead_decide(nbody_ctx* c, State<float>& s, AheadStep& a, float delta, PhaseEvents* chain) {
  HIPCHK(c, hipEventSynchronize(c->spec_event));
  if (int rc = step_ahead_collect<float>(c, s)) return rc;  // (the previous step's copies are older than this event)
  const StepAheadRecord& h = *c->spec_host;
  const int* flags = h.build;
  const int* bigcount = h.build + (a.L.bigcount - a.L.flags) / sizeof(int);  // the level counters, where the build's layout has them
  const int* info = h.info_before;
  if (env_int("NBODY_TRACE", 0) != 0) {
    std::fprintf(stderr, "[nbody] step ahead: build verdict %d (%d nodes, depth %d, fallback %d, %d blind levels)\n", h.verdict[1],
                 flags[kBvhNodes], flags[kBvhMaxDepth], flags[kBvhFallback], a.lv_end);
    std::fprintf(stderr, "[nbody] tile walk (step ahead): estimate from the last walk (shift %d, total %d), %d per wave, overflow %d\n", a.shift,
                 info[0], info[3], info[1]);
    trace_route("tile", &a.route, a.fused_scan ? "scan-tail" : "check-tail", true, s.n, false);
  }
  if (h.verdict[1] == 0) {  // the build needs more levels or the host builder
    s.wt_hist_n = -1;  // (the walk returned at once and left zeros in the history)
    s.bvh_levels_hint = s.bvh_levels_stable = 0;
    a.clock.give_up();  // (the plain sequence that follows books the step)
    return 1;
  }
  // the build stands: what bvh_build_device records
  record_bvh_levels(s, bigcount, true);
  commit_tree(c, s, NBODY_TREE_BVH, flags[kBvhNodes], flags[kBvhMaxDepth], flags[kBvhStops], true, true);
  c->last_build_device = true;
  s.ahead_total_due = info[1] == 0;  // (otherwise the estimate's scan wrapped and the walk kernel returned at once: walk again the plain way)
  if (!s.ahead_total_due)
    if (int rc = tree_walk_phase<float>(c, s, NBODY_TREE_BVH, self_targets(s, s.cur, NBODY_TREE_BVH, c->params.order), s.acc, bodies_walk(c, s)))
      return rc;
  Gate carry;  // the walk's info after the walk (its exact term count), read one step late: the integration's first threads take it along
  carry.carry_src = (const int*)(s.ws_scratch + a.WL.info);
  carry.carry_dst = c->spec_host_dev->info_after;
  carry.carry_words = sizeof(StepAheadRecord::info_after) / sizeof(int); carry.stamp = a.clock.stamp(2);
  HIPCHK(c, launch_integrate<float>(c->stream, s.set[s.cur].pos, s.set[s.cur].vel, s.acc, s.n, delta, carry));
  return a.clock.close(chain);  // (events: the next step starts where this one ends)
}

// Returns NBODY_OK (step done), 1 (not applicable / speculation failed: take the plain sequence), or an error.
template <class T> int bvh_step_ahead(nbody_ctx* c, State<T>& s, T delta, PhaseEvents* chain) {
  if constexpr (std::is_same<T, float>::value) {
    AheadStep a;
    int rc = step_ahead_applies(c, s, a);
    if (!rc) rc = step_ahead_enqueue(c, s, a, chain);
    if (!rc) rc = step_ahead_decide(c, s, a, delta, chain);
    return rc;
  }
  return 1;
}

// The tracers' share of a tree step (ctx.h, Tracers): the step's tree walked at the tracers' positions, after the bodies' walk
// and before anything is integrated (a BVH's leaves ARE the bodies' rows), in batches that bound the walk's scratch; then their
// integration behind the bodies'.  The timer and the walk statistics stay the bodies' alone, and so does ws_backoff — the batches
// move a copy of it: how many terms the tracers take says nothing about which walk suits the bodies.  (What the tracers' walk
// does displace is the bodies' history for the next walk's estimate — wt_hist_n — so that walk counts its terms instead; and
// each batch of a tile walk reads its `info` back, one host wait of the kind the bodies' walk has.)
constexpr int64_t kTracerWalkBatch = 1 << 20;
template <class T> int tracers_walk(nbody_ctx* c, State<T>& s, int kind) {
  using T2 = typename State<T>::T2;
  const Tracers& tr = c->tracers;
  int backoff = s.ws_backoff;
  int rc = NBODY_OK;
  for (int64_t b0 = 0; b0 < tr.m && !rc; b0 += kTracerWalkBatch)
    rc = tree_walk_phase<T>(c, s, kind, point_targets<T>((const T2*)tr.pos + b0, std::min<int64_t>(kTracerWalkBatch, tr.m - b0)), (T2*)tr.acc + b0,
                            WalkOpts{nullptr, false, &backoff});
  return rc;
}

// One step in the plain sequence — no host wait between the phases but those a phase needs for itself — over every row, or
// (count >= 0) a rank's slice [begin, begin + count) of the tree-ordered targets (update_tree_shard).
template <class T> int plain_tree_step(nbody_ctx* c, State<T>& s, int kind, T delta, int64_t begin = 0, int64_t count = -1) {
  StepClock clock;
  int rc = clock.begin(c, false);
  if (!rc) rc = tree_build_phase<T>(c, s, kind);
  if (!rc) rc = clock.mark(1);
  if (!rc) rc = tree_walk_phase<T>(c, s, kind, self_targets(s, s.cur, kind, c->params.order, begin, count), s.acc, bodies_walk(c, s));
  const bool tracers = count < 0 && c->tracers.m > 0;  // (a sharded step refuses them)
  if (!rc && tracers) rc = tracers_walk<T>(c, s, kind);
  if (!rc) rc = clock.mark(2);
  if (rc) return rc;
  auto& st = s.set[s.cur];
  if (count < 0) {
    hipError_t e = launch_integrate<T>(c->stream, st.pos, st.vel, s.acc, s.n, delta);
    if (e == hipSuccess && tracers) e = launch_integrate<T>(c->stream, c->tracers.pos, c->tracers.vel, c->tracers.acc, c->tracers.m, delta);
    if (e != hipSuccess) return fail_hip(c, e, "launch_integrate");
  } else {
    const uint32_t* rows = kind == NBODY_TREE_QUAD ? s.order_dev + begin : nullptr;
    hipError_t e = launch_integrate_rows<T>(c->stream, st.pos, st.vel, s.acc, rows, begin, count, delta);
    if (e != hipSuccess) return fail_hip(c, e, "launch_integrate_rows");
  }
  return clock.close();
}

// `async`: return once everything is enqueued (for a step ahead: once the host's one decision per step is made) instead of
// waiting for the last step; nbody_wait (or any call that reads the rows) completes it.
template <class T> int update_tree(nbody_ctx* c, int kind, T delta, int n_steps, nbody_counting* counter, bool async = false) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "update_tree: no particles of this precision uploaded");
  if (n_steps < 0) return fail(c, NBODY_ERR_INVALID, "update_tree: n_steps < 0");
  HIPCHK(c, hipSetDevice(c->device));
  State<T>& s = state_of<T>(c);
  c->phases.counter = counter;
  auto done = [&](int rc) {
    int rc2 = phase_drain(c);  // (waits for the last step: the call is synchronous)
    if (!rc2 && s.ahead_total_due) {
      hipError_t e = hipStreamSynchronize(c->stream);
      rc2 = e == hipSuccess ? step_ahead_collect<T>(c, s) : fail_hip(c, e, "hipStreamSynchronize");
    }
    c->phases.counter = nullptr;
    return rc ? rc : rc2;
  };
  PhaseEvents chain;  // the step before, when the next one follows it directly on the stream
  for (int step = 0; step < n_steps; ++step) {
    if (phase_backlog(c)) {
      int rc = phase_drain(c);
      if (rc) return done(rc);
      chain = PhaseEvents{};
    }
    if (kind == NBODY_TREE_BVH && c->tracers.m == 0) {  // (the step enqueued ahead does not carry the tracers' walk: the plain sequence, same bits)
      int rc = bvh_step_ahead<T>(c, s, delta, &chain);
      if (rc < 0) return done(rc);
      if (rc == NBODY_OK) {
        ++c->steps_done;
        continue;
      }
    }
    chain = PhaseEvents{};
    if (int rc = plain_tree_step<T>(c, s, kind, delta)) return done(rc);
    ++c->steps_done;
  }
  if (async) {  // the phase events and the last walk's term count are collected by nbody_wait or the next synchronous call
    // (a stamped step's end is written now: whatever the caller does before its next step is not this step's integration)
    if (int rc = close_open_stamp(c)) return rc;
    c->phases.counter = nullptr;
    return NBODY_OK;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return done(NBODY_OK);
}

// One tree step of a rank that owns the slice [begin, begin+count) of the tree-ordered targets: the tree is built over
// ALL particles (every rank holds them all and builds the same tree), the walk and the integration touch only the slice.
template <class T> int update_tree_shard(nbody_ctx* c, int kind, T delta, int64_t begin, int64_t count, nbody_counting* counter) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "update_tree_shard: no particles of this precision uploaded");
  State<T>& s = state_of<T>(c);
  if (begin < 0 || count < 0 || begin + count > s.n) return fail(c, NBODY_ERR_INVALID, "update_tree_shard: slice out of range");
  HIPCHK(c, hipSetDevice(c->device));
  c->phases.counter = counter;
  auto done = [&](int rc) {
    int rc2 = phase_drain(c);
    c->phases.counter = nullptr;
    return rc ? rc : rc2;
  };
  if (int rc = plain_tree_step<T>(c, s, kind, delta, begin, count)) return done(rc);
  s.shard_kind = kind;
  ++c->steps_done;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return done(NBODY_OK);
}
template <class T>
int export_slice(nbody_ctx* c, int64_t begin, int64_t count, void* rows_dev, void* pos_dev, void* vel_dev) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "export_slice: no particles of this precision uploaded");
  State<T>& s = state_of<T>(c);
  if (!s.tree_valid) return fail(c, NBODY_ERR_INVALID, "export_slice: no tree step yet");
  if (begin < 0 || count < 0 || begin + count > s.n || !rows_dev || !pos_dev || !vel_dev)
    return fail(c, NBODY_ERR_INVALID, "export_slice: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t* rows = s.shard_kind == NBODY_TREE_QUAD ? s.order_dev + begin : nullptr;
  HIPCHK(c, launch_export_rows<T>(c->stream, s.set[s.cur].pos, s.set[s.cur].vel, rows, begin, count, (uint32_t*)rows_dev, pos_dev, vel_dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}
template <class T> int import_rows_api(nbody_ctx* c, int64_t n_rows, const void* rows_dev, const void* pos_dev, const void* vel_dev) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "import_rows: no particles of this precision uploaded");
  State<T>& s = state_of<T>(c);
  if (n_rows < 0 || (n_rows > 0 && (!rows_dev || !pos_dev || !vel_dev))) return fail(c, NBODY_ERR_INVALID, "import_rows: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_import_rows<T>(c->stream, s.set[s.cur].pos, s.set[s.cur].vel, (const uint32_t*)rows_dev, n_rows, s.n, pos_dev, vel_dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  s.tree_valid = false;
  return NBODY_OK;
}

}  // namespace

template <class T> int accel_built_tree(nbody_ctx* c, State<T>& s, int kind, int64_t n_targets, const T* target_xy, T* acc_xy) {
  using T2 = typename State<T>::T2;
  int rc = NBODY_OK;
  if (!target_xy) {
    // particles themselves, post-build row order, regardless of params.order
    WalkTargets<T> t = self_targets(s, s.cur, kind, NBODY_ORDER_CONSISTENT);
    if (kind == NBODY_TREE_BVH) t.ids = nullptr;  // (walked as points at the rows' places: neither uses nor leaves a history)
    rc = tree_walk_phase<T>(c, s, kind, t, s.acc, bodies_walk(c, s));
    if (rc) return rc;
    if (s.n) HIPCHK(c, hipMemcpyAsync(acc_xy, s.acc, (size_t)s.n * sizeof(T2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NBODY_OK;
  }
  if (n_targets < 0) return fail(c, NBODY_ERR_INVALID, "accel_tree: n_targets < 0");
  if (n_targets == 0) return NBODY_OK;
  T2 *tp = nullptr, *ta = nullptr;
  HIPCHK(c, hipMalloc((void**)&tp, (size_t)n_targets * sizeof(T2)));
  hipError_t e = hipMalloc((void**)&ta, (size_t)n_targets * sizeof(T2));
  if (e != hipSuccess) { (void)hipFree(tp); return fail_hip(c, e, "hipMalloc"); }
  e = hipMemcpyAsync(tp, target_xy, (size_t)n_targets * sizeof(T2), hipMemcpyHostToDevice, c->stream);
  rc = (e == hipSuccess) ? tree_walk_phase<T>(c, s, kind, point_targets<T>(tp, n_targets), ta, bodies_walk(c, s)) : fail_hip(c, e, "hipMemcpyAsync");
  if (!rc) {
    e = hipMemcpyAsync(acc_xy, ta, (size_t)n_targets * sizeof(T2), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail_hip(c, e, "download acc");
  }
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(tp);
  (void)hipFree(ta);
  return rc;
}

template int accel_built_tree<float>(nbody_ctx*, State<float>&, int, int64_t, const float*, float*);
template int accel_built_tree<double>(nbody_ctx*, State<double>&, int, int64_t, const double*, double*);

namespace {
template <class T> int accel_tree(nbody_ctx* c, int kind, int64_t n_targets, const T* target_xy, T* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "accel_tree: no particles of this precision uploaded");
  if (!acc_xy) return fail(c, NBODY_ERR_INVALID, "accel_tree: acc_xy is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  State<T>& s = state_of<T>(c);
  int rc = tree_build_phase<T>(c, s, kind);
  if (rc) return rc;
  return accel_built_tree<T>(c, s, kind, n_targets, target_xy, acc_xy);
}
// ... the walk alone, over the tree that is installed (the library's build or a caller's tree)
}  // namespace
}  // namespace nbody

using namespace nbody;

static int not_with_tracers(nbody_ctx* c, const char* what) {
  return fail(c, NBODY_ERR_INVALID, std::string(what) + ": not available while the context holds tracers (nbody_tracers_upload_*)");
}

NB_API int nbody_update_tree_f32(nbody_ctx* c, int kind, float delta, int n_steps, nbody_counting* counter) {
  if (c && c->multi) return nbody::multi_update_tree(c, false, kind, (double)delta, n_steps, counter);
  return update_tree<float>(c, kind, delta, n_steps, counter);
}
NB_API int nbody_update_tree_f64(nbody_ctx* c, int kind, double delta, int n_steps, nbody_counting* counter) {
  if (c && c->multi) return nbody::multi_update_tree(c, true, kind, delta, n_steps, counter);
  return update_tree<double>(c, kind, delta, n_steps, counter);
}
// Asynchronous form of nbody_update_tree_f32 and its completion.
NB_API int nbody_update_tree_async_f32(nbody_ctx* c, int kind, float delta, int n_steps) {
  if (c && c->multi) return nbody::multi_update_tree(c, false, kind, (double)delta, n_steps, nullptr);  // (synchronous there)
  if (c && c->tracers.m > 0) return not_with_tracers(c, "update_tree_async");
  return update_tree<float>(c, kind, delta, n_steps, nullptr, true);
}
NB_API int nbody_wait(nbody_ctx* c) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return NBODY_OK;  // every call on a multi-device context is synchronous
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = phase_drain(c);
  if (!rc && c->has_f32) rc = step_ahead_collect<float>(c, c->sf);
  return rc;
}
static int not_on_multi(nbody_ctx* c, const char* what) {
  return fail(c, NBODY_ERR_INVALID, std::string(what) + ": a context made by nbody_create_multi shards its steps itself");
}
NB_API int nbody_update_tree_shard_f32(nbody_ctx* c, int kind, float delta, int64_t begin, int64_t count, nbody_counting* counter) {
  if (c && c->multi) return not_on_multi(c, "update_tree_shard");
  if (c && c->tracers.m > 0) return not_with_tracers(c, "update_tree_shard");
  return update_tree_shard<float>(c, kind, delta, begin, count, counter);
}
NB_API int nbody_update_tree_shard_f64(nbody_ctx* c, int kind, double delta, int64_t begin, int64_t count, nbody_counting* counter) {
  if (c && c->multi) return not_on_multi(c, "update_tree_shard");
  if (c && c->tracers.m > 0) return not_with_tracers(c, "update_tree_shard");
  return update_tree_shard<double>(c, kind, delta, begin, count, counter);
}
NB_API int nbody_export_slice_dev(nbody_ctx* c, int64_t begin, int64_t count, void* rows_u32, void* pos_xy, void* vel_xy) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return not_on_multi(c, "export_slice");
  if (c && c->tracers.m > 0) return not_with_tracers(c, "export_slice");
  return c->has_f64 ? export_slice<double>(c, begin, count, rows_u32, pos_xy, vel_xy)
                    : export_slice<float>(c, begin, count, rows_u32, pos_xy, vel_xy);
}
NB_API int nbody_import_rows_dev(nbody_ctx* c, int64_t n_rows, const void* rows_u32, const void* pos_xy, const void* vel_xy) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return not_on_multi(c, "import_rows");
  if (c && c->tracers.m > 0) return not_with_tracers(c, "import_rows");
  return c->has_f64 ? import_rows_api<double>(c, n_rows, rows_u32, pos_xy, vel_xy)
                    : import_rows_api<float>(c, n_rows, rows_u32, pos_xy, vel_xy);
}
// (a BVH build permutes the rows of the device that ran it: the other replicas are refreshed afterwards)
NB_API int nbody_accel_tree_f32(nbody_ctx* c, int kind, int64_t n_targets, const float* target_xy, float* acc_xy) {
  NB_VIA_PRIMARY(c, true, accel_tree<float>(p, kind, n_targets, target_xy, acc_xy));
  return accel_tree<float>(c, kind, n_targets, target_xy, acc_xy);
}
NB_API int nbody_accel_tree_f64(nbody_ctx* c, int kind, int64_t n_targets, const double* target_xy, double* acc_xy) {
  NB_VIA_PRIMARY(c, true, accel_tree<double>(p, kind, n_targets, target_xy, acc_xy));
  return accel_tree<double>(c, kind, n_targets, target_xy, acc_xy);
}
NB_API int nbody_tree_walk_stats(nbody_ctx* c, int enable, uint64_t* node_visits, uint64_t* accepted, uint64_t* leaf_pairs) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return not_on_multi(c, "tree_walk_stats (each device walks a slice)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (node_visits) *node_visits = c->last_stats[0];
  if (accepted) *accepted = c->last_stats[1];
  if (leaf_pairs) *leaf_pairs = c->last_stats[2];
  c->want_stats = enable != 0;
  return NBODY_OK;
}

// ---- what multi.hip needs of this translation unit (ctx.h)
namespace nbody {
int ctx_update_tree(nbody_ctx* c, bool f64, int kind, double delta, int n_steps, nbody_counting* counter) {
  return f64 ? update_tree<double>(c, kind, delta, n_steps, counter) : update_tree<float>(c, kind, (float)delta, n_steps, counter);
}
int ctx_update_tree_shard(nbody_ctx* c, bool f64, int kind, double delta, int64_t begin, int64_t count, nbody_counting* counter) {
  return f64 ? update_tree_shard<double>(c, kind, delta, begin, count, counter)
             : update_tree_shard<float>(c, kind, (float)delta, begin, count, counter);
}
int ctx_export_slice(nbody_ctx* c, int64_t begin, int64_t count, void* rows, void* pos, void* vel) {
  return c->has_f64 ? export_slice<double>(c, begin, count, rows, pos, vel) : export_slice<float>(c, begin, count, rows, pos, vel);
}
int ctx_import_rows(nbody_ctx* c, int64_t n_rows, const void* rows, const void* pos, const void* vel) {
  return c->has_f64 ? import_rows_api<double>(c, n_rows, rows, pos, vel) : import_rows_api<float>(c, n_rows, rows, pos, vel);
}
}  // namespace nbody
