// Internal: the host plumbing the single-device driver's translation units share (capi.hip, direct_driver.hip, target_driver.hip,
// tree_build_driver.hip, tree_driver.hip, caller_tree.hip, snapshot.hip) — error reporting, device buffers, and the
// bookkeeping every tree build and walk repeats.  Not part of the C ABI; multi.hip needs only ctx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

#include "bvh_build.h"
#include "ctx.h"
#include "fast_domain.h"
#include "tree_kernels.h"

#define NB_API extern "C" __attribute__((visibility("default")))

namespace nbody {

int fail(nbody_ctx* c, int code, const std::string& msg);  // c == NULL: the thread's create error (capi.hip)
inline int fail_hip(nbody_ctx* c, hipError_t e, const char* what) {
  return fail(c, NBODY_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(c, call)                                   \
  do {                                                    \
    hipError_t e__ = (call);                              \
    if (e__ != hipSuccess) return fail_hip(c, e__, #call); \
  } while (0)

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class P> void free_dev(P*& p) { if (p) (void)hipFree((void*)p); p = nullptr; }
template <class P> void free_host(P*& p) { if (p) (void)hipHostFree((void*)p); p = nullptr; }  // (pinned)
// A device buffer of at least `need` bytes; a smaller one is freed and replaced (its contents are not kept).
template <class P> int ensure_dev_bytes(nbody_ctx* c, P*& p, size_t& bytes, size_t need) {
  if (bytes >= need) return NBODY_OK;
  free_dev(p);
  bytes = 0;
  HIPCHK(c, hipMalloc((void**)&p, need));
  bytes = need;
  return NBODY_OK;
}

template <class T> State<T>& state_of(nbody_ctx* c);
template <> inline State<float>& state_of<float>(nbody_ctx* c) { return c->sf; }
template <> inline State<double>& state_of<double>(nbody_ctx* c) { return c->sd; }
template <class T> bool has_state(const nbody_ctx* c);
template <> inline bool has_state<float>(const nbody_ctx* c) { return c->has_f32; }
template <> inline bool has_state<double>(const nbody_ctx* c) { return c->has_f64; }

// ---- tree bookkeeping
// The rows set[cur] gathered into set[1 - cur] in the order `perm`, every column: as the in-place partition leaves
// `self.particles` (bvh_tree.rs:73-77).  The quad tree's leaf copies clear the outputs they do not need.
template <class T> GatherArgs<T> row_gather_args(const State<T>& s, const uint32_t* perm) {
  const auto& in = s.set[s.cur];
  const auto& out = s.set[1 - s.cur];
  GatherArgs<T> g{};
  g.perm = perm;
  g.n = s.n;
  g.pos_in = in.pos; g.pos_out = out.pos;
  g.vel_in = in.vel; g.vel_out = out.vel;
  g.weight_in = in.weight; g.weight_out = out.weight;
  g.ids_in = in.ids; g.ids_out = out.ids;
  g.mass_out = out.mass;
  return g;
}

// A finished build becomes the context's tree.  `rows_permuted`: the build gathered the rows into tree order in set[1 - cur],
// which becomes the current set (a BVH; the quad tree leaves the rows where they are).  `on_device`: the host has neither
// the tree nor, for permuted rows, the weights in their new order.
template <class T>
void commit_tree(nbody_ctx* c, State<T>& s, int kind, int n_nodes, int max_depth, int stops, bool rows_permuted, bool on_device) {
  if (rows_permuted) {
    s.cur = 1 - s.cur;
    ++s.row_epoch;
    if (on_device) s.h_weight_stale = true;
  }
  s.n_nodes = n_nodes;
  s.tree_kind = kind;
  s.tree_max_depth = max_depth;
  s.tree_host_stale = on_device;
  s.tree_valid = true;
  c->bvh_stops = stops;
}

// How many long-node levels a device-built BVH had (`bigcount`: the build's level counters): what a step enqueued ahead
// of the host enqueues blind next time.  A step-ahead build (`ahead`) counts the builds for which that number has
// stood (bvh_step_ahead drops its spare level after eight); any other build starts that count again.
template <class T> void record_bvh_levels(State<T>& s, const int* bigcount, bool ahead) {
  int used = 0;
  while (used < kBvhLevels - 1 && bigcount[used] != 0) ++used;
  s.bvh_levels_stable = (ahead && used == s.bvh_levels_hint) ? s.bvh_levels_stable + 1 : 0;
  s.bvh_levels_hint = used;
}

static_assert(kBvhFlagWords + kBvhLevels <= kAheadBuildWords, "flags and level counters travel as one 512-byte block (StepAheadRecord)");

// The f32 device BVH build enqueued blind (tree_build_driver.hip), as bvh_build_device and bvh_step_ahead both do it.
// How many long-node levels go first: as many as the last tree had (`hint`, 0: unknown — then a balanced tree's, plus two: a
// lopsided tree has more), plus one.  The spare level is four launches that find nothing to do (19 us of a 1.1 ms step): once the
// count has stood for eight builds (`stable`) it is dropped — the verdict still checks that no long node is left, and a tree that
// grows a level then costs ONE repeated step and brings the spare back.  0: no long-node level at all.  (NBODY_BVH_BLIND_LEVELS,
// laboratory: tests force too few levels.)
int bvh_blind_levels(int64_t n, int hint, int stable);
// ... and its tail: subtrees, numbering, and — in the numbering's launch — the row gather into set[1 - cur], the permutation
// read where the build left it and copied out to order_dev on the way.  `zero8` (optional): eight words that launch clears too.
int bvh_finish_gather(nbody_ctx* c, State<float>& s, const BvhBuildLayout& L, int sub_start, int* zero8 = nullptr);

// "The bodies themselves" as the targets of a walk over the tree of `kind`, all of them or (count >= 0) the slice
// [begin, begin + count) of the tree-ordered targets.  `rows`: which set holds the rows in tree order (s.cur once a build is
// committed).  BVH under AS_WRITTEN: accelerations are computed for the snapshot's rows (main.rs:406-412 iterate `cloned`; tree
// order = row order after the build's permutation), the other set; the quad tree reaches its rows through the order.
template <class T> struct WalkTargets {
  const void* pos = nullptr;
  int64_t n = 0;
  int64_t first = 0;                // the slice's first target
  int64_t acc_first = 0;            // ... and where in `acc` its results start (the quad tree's go through the index)
  const uint32_t* index = nullptr;  // quad tree: target t is row index[t]
  const uint32_t* ids = nullptr;    // the targets' particle ids; nullptr: the targets are not the bodies
};
template <class T> WalkTargets<T> self_targets(const State<T>& s, int rows, int kind, int order, int64_t begin = 0, int64_t count = -1) {
  const auto& as_rows = s.set[order == NBODY_ORDER_AS_WRITTEN ? 1 - rows : rows];
  WalkTargets<T> t;
  t.first = count >= 0 ? begin : 0;
  t.n = count >= 0 ? count : s.n;
  t.ids = as_rows.ids + t.first;
  if (kind == NBODY_TREE_BVH) { t.pos = as_rows.pos + t.first; t.acc_first = t.first; }
  else { t.pos = s.set[rows].pos; t.index = s.order_dev + t.first; }
  return t;
}
template <class T> WalkTargets<T> point_targets(const void* pos, int64_t n) {  // any other points (device memory)
  WalkTargets<T> t;
  t.pos = pos;
  t.n = n;
  return t;
}
// What a walk takes from its caller besides the targets (tree_driver.hip, tree_walk_phase).  The bodies' walk: the context's
// timer and statistics, the state's back-off.
struct WalkOpts {
  nbody_timer* timer = nullptr;  // times the walk kernels
  bool stats = false;            // the walk statistics are collected (by the fused walk: the others do not count)
  int* backoff = nullptr;        // walks for which the split walks are not tried: read, and moved, through here
};
template <class T> WalkOpts bodies_walk(nbody_ctx* c, State<T>& s) { return WalkOpts{c->timer, c->want_stats, &s.ws_backoff}; }

// The walk's parameters and tree arrays; the caller sets the leaves, the targets, `acc` and the node count.
template <class T> WalkArgs<T> walk_args(const nbody_ctx* c, const State<T>& s, int kind) {
  WalkArgs<T> w{};
  w.geom0 = s.geom0; w.geom1 = s.geom1; w.link = s.link;
  w.big_leaves = kind == NBODY_TREE_BVH && c->params.leaf_size >= 16;
  w.fast = c->params.arith == NBODY_ARITH_FAST;  // AUTO and EXACT walk with the reference's operations
  w.theta = (T)c->params.theta;
  w.clamp = (T)c->params.clamp;
  return w;
}

// The arithmetic a direct sum runs in under the context's params.  f32: FAST and AUTO need the clamp floor of fast_domain.h (a
// smaller clamp, or a NaN, takes EXACT).  f64: FAST only where it is asked for, with a clamp > 0 (a NaN fails the test too).
inline int direct_arith_f32(int arith, float clamp) {
  return arith != NBODY_ARITH_EXACT && !(clamp >= kFastClampFloor) ? (int)NBODY_ARITH_EXACT : arith;
}
inline bool direct_fast_f64(int arith, double clamp) { return arith == NBODY_ARITH_FAST && clamp > 0.0; }

// ---- shared between the translation units
void free_snapshot(nbody_ctx* c);  // snapshot.hip
void free_delta(nbody_ctx* c);
template <class T> int refresh_host_weights(nbody_ctx* c, State<T>& s);  // tree_build_driver.hip
template <class T> int install_host_tree(nbody_ctx* c, State<T>& s, int kind);
template <class T> int tree_build_phase(nbody_ctx* c, State<T>& s, int kind);
template <class T> int download_tree(nbody_ctx* c, State<T>& s);
template <class T>  // tree_driver.hip
int accel_built_tree(nbody_ctx* c, State<T>& s, int kind, int64_t n_targets, const T* target_xy, T* acc_xy);
// target_driver.hip: the tracers' share of one direct step, enqueued behind the bodies' kernels of that step and before its buffers
// swap (`pos` / `mass`: the bodies at their pre-step positions)
int tracers_direct_f32(nbody_ctx* c, const float2* pos, const float* mass, float delta);
int tracers_direct_f64(nbody_ctx* c, const double2* pos, const double* mass, double delta);

}  // namespace nbody

// A handle made by nbody_create_multi fronts several devices.  Calls that only read or that act on "the current rows"
// are served by the first device once the replicas agree (multi_primary brings them up to date); `mutates` marks the
// calls after which the other replicas must be refreshed from it (multi_replicate).
#define NB_VIA_PRIMARY(c, mutates, expr)                    \
  do {                                                      \
    if ((c) && (c)->multi) {                                \
      nbody_ctx* front__ = (c);                             \
      nbody_ctx* p = nullptr;                               \
      int rc__ = nbody::multi_primary(front__, &p);         \
      if (rc__) return rc__;                                \
      rc__ = (expr);                                        \
      if (rc__) { front__->err = p->err; return rc__; }     \
      return (mutates) ? nbody::multi_replicate(front__) : NBODY_OK; \
    }                                                       \
  } while (0)
