// libnbody_hip — phase 1 of a tree step (main.rs:398-401): the device builds (BVH in f32 and f64, quad tree), the host
// builders' fallback and the installation of a linearised tree (the host builders', or a caller's: caller_tree.hip), and the
// host image of a device-built tree for the export API.  Kernels: bvh_build.hip (with bvh_fold / bvh_partition / bvh_subtrees / bvh_finish.hip), bvh_build64.hip, quad_build.hip, tree_kernels.hip.
#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "bvh_build.h"
#include "bvh_build64.h"
#include "driver.h"
#include "quad_build.h"
#include "tree_build.hpp"

namespace nbody {
namespace {

template <class T> int ensure_node_buffers(nbody_ctx* c, State<T>& s, size_t m) {
  using G4 = typename TreeHost<T>::G4;
  using L4 = typename TreeHost<T>::L4;
  if (m > s.node_cap) {
    free_dev(s.geom0); free_dev(s.geom1); free_dev(s.link);
    s.node_cap = 0;
    size_t cap = m + m / 4 + 64;
    HIPCHK(c, hipMalloc(&s.geom0, cap * sizeof(G4)));
    HIPCHK(c, hipMalloc(&s.geom1, cap * sizeof(G4)));
    HIPCHK(c, hipMalloc(&s.link, cap * sizeof(L4)));
    s.node_cap = cap;
  }
  return NBODY_OK;
}

template <class T> int upload_tree(nbody_ctx* c, State<T>& s) {
  const size_t m = s.tree.size();
  using G4 = typename TreeHost<T>::G4;
  using L4 = typename TreeHost<T>::L4;
  int rc0 = ensure_node_buffers<T>(c, s, m);
  if (rc0) return rc0;
  HIPCHK(c, hipMemcpyAsync(s.geom0, s.tree.geom0.data(), m * sizeof(G4), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(s.geom1, s.tree.geom1.data(), m * sizeof(G4), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(s.link, s.tree.link.data(), m * sizeof(L4), hipMemcpyHostToDevice, c->stream));
  if (s.n) HIPCHK(c, hipMemcpyAsync(s.order_dev, s.tree.order.data(), (size_t)s.n * 4, hipMemcpyHostToDevice, c->stream));
  return NBODY_OK;
}

// ... and the per-node arrays a device build writes beside them
template <class T> int ensure_node_aux(nbody_ctx* c, State<T>& s, size_t m) {
  if (int rc = ensure_node_buffers<T>(c, s, m)) return rc;
  if (m > s.node_aux_cap) {
    free_dev(s.node_depth); free_dev(s.node_mass); free_dev(s.node_size);
    s.node_aux_cap = 0;
    size_t cap = m + m / 4 + 64;
    HIPCHK(c, hipMalloc((void**)&s.node_depth, cap * sizeof(int)));
    HIPCHK(c, hipMalloc((void**)&s.node_mass, cap * sizeof(uint32_t)));
    HIPCHK(c, hipMalloc((void**)&s.node_size, cap * sizeof(typename State<T>::T2)));
    s.node_aux_cap = cap;
  }
  return NBODY_OK;
}

// BVH built on the device (bvh_build.hip and its units, f32 only).  Returns NBODY_OK, an error, or 1 when the device build declines.
// The same for f64 rows (bvh_build64.hip): every level enqueued blind, one question at the end.
int bvh_build_device64(nbody_ctx* c, State<double>& s) {
  const int n = (int)s.n;
  const int leaf = c->params.leaf_size;
  const Bvh64Layout L = bvh64_layout(n, leaf);
  int rc = ensure_dev_bytes(c, s.bb_scratch, s.bb_scratch_bytes, L.total);
  if (rc) return rc;
  rc = ensure_node_aux<double>(c, s, (size_t)L.node_cap);
  if (rc) return rc;
  auto& in = s.set[s.cur];
  HIPCHK(c, bvh64_begin(c->stream, in.pos, n, s.bb_scratch, L));
  // the levels a balanced tree has, plus a margin (the mean split is not the median: real trees run a few levels deeper);
  // a tree that is deeper still goes on four levels at a time
  int lv_end = std::min(bvh64_first_levels(n, leaf) + 4, kB64Levels);
  lv_end = std::max(1, std::min(lab_int("NBODY_BVH_BLIND_LEVELS", lv_end), kB64Levels));  // tests force the long way
  int hostf[kB64FlagWords + kB64Levels + 2];
  auto finish_and_ask = [&]() -> int {
    HIPCHK(c, bvh64_finish(c->stream, in.weight, n, lv_end, s.bb_scratch, L, s.order_dev, s.geom0, s.geom1, s.link, s.node_depth, s.node_mass,
                           s.node_size));
    HIPCHK(c, hipMemcpyAsync(hostf, s.bb_scratch + L.flags, kB64FlagWords * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hostf + kB64FlagWords, s.bb_scratch + L.opencount, (kB64Levels + 2) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NBODY_OK;
  };
  HIPCHK(c, bvh64_levels(c->stream, n, leaf, 0, lv_end, s.bb_scratch, L));
  rc = finish_and_ask();
  if (rc) return rc;
  while (hostf[kB64Fallback] == 0 && hostf[kB64FlagWords + lv_end] != 0) {  // open nodes were left behind
    if (lv_end >= kB64Levels) return 1;  // deeper than the device follows (coincident points): the host builder reports it
    const int lv = lv_end;
    lv_end = std::min(lv_end + 4, kB64Levels);
    HIPCHK(c, bvh64_levels(c->stream, n, leaf, lv, lv_end, s.bb_scratch, L));
    rc = finish_and_ask();
    if (rc) return rc;
  }
  if (env_int("NBODY_TRACE", 0) != 0)
    std::fprintf(stderr, "[nbody] device bvh build (f64): %d nodes, depth %d, %d levels enqueued, %d scan restarts, %d prepared runs used, fallback %d\n",
                 hostf[kB64NodeCount], hostf[kB64MaxDepth], lv_end, hostf[kB64Stops], hostf[kB64RunsUsed], hostf[kB64Fallback]);
  const int m = hostf[kB64NodeCount];
  if (hostf[kB64Fallback] != 0 || m <= 0 || m > L.node_cap) return 1;
  HIPCHK(c, launch_gather<double>(c->stream, row_gather_args(s, s.order_dev)));
  commit_tree(c, s, NBODY_TREE_BVH, m, hostf[kB64MaxDepth], hostf[kB64Stops], true, true);
  return NBODY_OK;
}

template <class T> int bvh_build_device(nbody_ctx* c, State<T>& s) {
  if constexpr (!std::is_same<T, float>::value) {
    return env_int("NBODY_TREE_BUILD_HOST", 0) != 0 ? 1 : bvh_build_device64(c, s);
  } else {
    const int n = (int)s.n;
    const int leaf = c->params.leaf_size;
    BvhBuildLayout L = bvh_build_layout(n, leaf);
    int rc = ensure_dev_bytes(c, s.bb_scratch, s.bb_scratch_bytes, L.total);
    if (rc) return rc;
    auto& in = s.set[s.cur];
    s.bb_flags_clean = false;
    HIPCHK(c, bvh_build_begin(c->stream, in.pos, n, s.bb_scratch, L));
    rc = ensure_node_aux<T>(c, s, (size_t)L.node_cap);
    if (rc) return rc;
    // Everything is enqueued blind — the long-node levels a balanced tree has (plus two), the subtrees, the numbering,
    // the row gather — and checked once at the end: asking in between costs a round trip per question, an empty level
    // a few microseconds.  A lopsided tree still has long nodes then: levels two at a time (asking after each pair)
    // until none is left, then the tail once more for the subtrees that were not there the first time.
    int lv_end = bvh_blind_levels(n, 0, 0);
    int hostf[kBvhFlagWords + kBvhLevels];
    auto tail = [&](int sub_start) -> int { return bvh_finish_gather(c, s, L, sub_start); };
    auto ask = [&]() -> int {
      HIPCHK(c, hipMemcpyAsync(hostf, s.bb_scratch + L.flags, kBvhFlagWords * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(hostf + kBvhFlagWords, s.bb_scratch + L.bigcount, kBvhLevels * sizeof(int), hipMemcpyDeviceToHost,
                               c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      return hostf[kBvhFallback] != 0 ? 1 : NBODY_OK;  // (1: the device build declines)
    };
    if (lv_end > 0) HIPCHK(c, bvh_build_levels(c->stream, n, leaf, 0, lv_end, s.bb_scratch, L));
    if ((rc = tail(0)) || (rc = ask())) return rc;
    if (lv_end > 0 && hostf[kBvhFlagWords + lv_end] != 0) {  // long nodes were left behind
      const int sub_start = hostf[kBvhSubCount];
      while (hostf[kBvhFlagWords + lv_end] != 0) {
        if (lv_end >= kBvhKeyDepth + 1) return 1;
        const int lv = lv_end;
        lv_end = lv_end + 2 > kBvhKeyDepth + 1 ? kBvhKeyDepth + 1 : lv_end + 2;
        HIPCHK(c, bvh_build_levels(c->stream, n, leaf, lv, lv_end, s.bb_scratch, L));
        if ((rc = ask())) return rc;
      }
      if ((rc = tail(sub_start)) || (rc = ask())) return rc;
    }
    if (env_int("NBODY_TRACE", 0) != 0)
      std::fprintf(stderr, "[nbody] device bvh build: %d nodes, depth %d, %d subtrees, %d long-node levels, %d scan restarts, %d prepared chunk runs used\n",
                   hostf[kBvhNodes], hostf[kBvhMaxDepth], hostf[kBvhSubCount], lv_end, hostf[kBvhStops], hostf[kBvhRunsUsed]);
#ifdef NB_BVH_TIMING
    std::fprintf(stderr, "[nbody] bvh_subtrees, slowest group per phase (10 ns ticks): load %d, level 1 %d, level 2 %d, level 3 %d, other levels %d, leaves %d, upward %d, store %d\n",
                 hostf[kBvhDebug], hostf[kBvhDebug + 1], hostf[kBvhDebug + 2], hostf[kBvhDebug + 3], hostf[kBvhDebug + 4], hostf[kBvhDebug + 5],
                 hostf[kBvhDebug + 6], hostf[kBvhDebug + 7]);
#endif
    const int m = hostf[kBvhNodes];
    if (m <= 0 || m > L.node_cap || hostf[kBvhNodeCount] > L.node_cap || hostf[kBvhBadIndex] != 0) return 1;
    record_bvh_levels(s, hostf + kBvhFlagWords, false);
    commit_tree(c, s, NBODY_TREE_BVH, m, hostf[kBvhMaxDepth], hostf[kBvhStops], true, true);
    return NBODY_OK;
  }
}

// Quad tree built on the device (quad_build.hip).  Returns NBODY_OK, an error, or 1 when the device build declines.
template <class T> int quad_build_device(nbody_ctx* c, State<T>& s) {
  const int n = (int)s.n;
  QuadBuildLayout L = quad_build_layout(n);
  int rc = ensure_dev_bytes(c, s.qb_scratch, s.qb_scratch_bytes, L.total);
  if (rc) return rc;
  auto& in = s.set[s.cur];
  auto& out = s.set[1 - s.cur];
  const T rx = (T)c->params.quad_root_x, ry = (T)c->params.quad_root_y, rh = (T)c->params.quad_root_h;
  // the sorts only look at as many levels as the tree is expected to have: the last quad tree's depth plus three (all 31
  // the first time, and again whenever that turns out to be too few; never more than the 31 the key holds, which is what
  // the trace then says)
  int sort_levels = s.quad_depth_hint > 0 ? std::min(s.quad_depth_hint + 3, 31) : 31;
  int flags[3] = {0, 0, 0};
  for (;;) {
    HIPCHK(c, quad_build_phase_a<T>(c->stream, in.pos, n, rx, ry, rh, s.qb_scratch, L, s.order_dev, sort_levels));
    HIPCHK(c, hipMemcpyAsync(flags, s.qb_scratch + L.flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    {
      // The leaves' own copies of their points, in tree order: enqueued before the host asks for the node count, so the
      // device gathers while the host waits, and the leaf statistics of phase B read rows that lie side by side.
      GatherArgs<T> g = row_gather_args(s, s.order_dev);
      g.vel_out = nullptr;
      g.ids_out = nullptr;
      HIPCHK(c, launch_gather<T>(c->stream, g));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (env_int("NBODY_TRACE", 0) != 0)
      std::fprintf(stderr, "[nbody] device quad build: sorted by %d levels, flags %d, %d nodes, depth %d\n", sort_levels, flags[0], flags[1], flags[2]);
    if ((flags[0] & 2) != 0 && sort_levels < 31) { sort_levels = 31; continue; }
    break;
  }
  if ((flags[0] & 1) != 0 || flags[1] <= 0) { s.quad_depth_hint = 0; return 1; }
  s.quad_depth_hint = flags[2];
  const int m = flags[1];
  rc = ensure_node_aux<T>(c, s, (size_t)m);
  if (rc) return rc;
  HIPCHK(c, quad_build_phase_b<T>(c->stream, out.pos, out.weight, n, rx, ry, rh, s.qb_scratch, L, nullptr, m, flags[2],
                                  s.geom0, s.geom1, s.link, s.node_depth, s.node_mass));
  commit_tree(c, s, NBODY_TREE_QUAD, m, flags[2], c->bvh_stops, false, true);
  return NBODY_OK;
}

}  // namespace

int bvh_blind_levels(int64_t n, int hint, int stable) {
  const int first_levels = bvh_build_first_levels(n);
  int lv_end = first_levels > 0 ? first_levels + 2 : 0;
  if (lv_end > 0 && hint > 0) lv_end = hint + ((stable >= 8 && lab_int("NBODY_BVH_SPARE_LEVEL", 0) == 0) ? 0 : 1);
  if (lv_end > 0) lv_end = std::max(1, lab_int("NBODY_BVH_BLIND_LEVELS", lv_end));
  return std::min(lv_end, kBvhKeyDepth + 1);
}
int bvh_finish_gather(nbody_ctx* c, State<float>& s, const BvhBuildLayout& L, int sub_start, int* zero8) {
  GatherArgs<float> g = row_gather_args(s, bvh_build_order(s.bb_scratch, L));
  g.perm_copy = s.order_dev;
  g.zero8 = zero8;
  HIPCHK(c, bvh_build_finish(c->stream, s.set[s.cur].weight, (int)s.n, c->params.leaf_size, sub_start, s.bb_scratch, L, nullptr, s.geom0,
                             s.geom1, s.link, s.node_depth, s.node_mass, s.node_size, &g));
  return NBODY_OK;
}

// Host image of a device-built tree, for the export API.
template <class T> int download_tree(nbody_ctx* c, State<T>& s) {
  if (!s.tree_host_stale) return NBODY_OK;
  using G4 = typename TreeHost<T>::G4;
  using L4 = typename TreeHost<T>::L4;
  const size_t m = (size_t)s.n_nodes;
  auto& t = s.tree;
  t.clear();
  t.kind = s.tree_kind;
  t.max_depth = s.tree_max_depth;
  t.geom0.resize(m); t.geom1.resize(m); t.link.resize(m); t.mass_u32.resize(m); t.order.resize((size_t)s.n);
  HIPCHK(c, hipMemcpyAsync(t.geom0.data(), s.geom0, m * sizeof(G4), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.geom1.data(), s.geom1, m * sizeof(G4), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.link.data(), s.link, m * sizeof(L4), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.mass_u32.data(), s.node_mass, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (s.n) HIPCHK(c, hipMemcpyAsync(t.order.data(), s.order_dev, (size_t)s.n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  t.size_x.resize(m); t.size_y.resize(m);
  if (s.tree_kind == NBODY_TREE_BVH) {  // boundary.size as the build computed it (max - min)
    std::vector<typename State<T>::T2> sz(m);
    HIPCHK(c, hipMemcpy(sz.data(), s.node_size, m * sizeof(typename State<T>::T2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; ++i) { t.size_x[i] = (T)sz[i].x; t.size_y[i] = (T)sz[i].y; }
    s.tree_host_stale = false;
    return NBODY_OK;
  }
  {  // height is not stored on the device; hi - lo would round.  Recover it exactly from the parent chain:
     // a child's height is its parent's height / 2 (quad_tree.rs:172), the root's is the parameter.
    std::vector<int> depth(m);
    HIPCHK(c, hipMemcpy(depth.data(), s.node_depth, m * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<T> hd((size_t)t.max_depth + 2);
    hd[0] = (T)c->params.quad_root_h;
    for (size_t d = 1; d < hd.size(); ++d) hd[d] = hd[d - 1] / (T)2.0;
    for (size_t i = 0; i < m; ++i) t.size_x[i] = t.size_y[i] = hd[(size_t)depth[i]];
  }
  s.tree_host_stale = false;
  return NBODY_OK;
}

// The host's mirror of the weights, in the current row order.
template <class T> int refresh_host_weights(nbody_ctx* c, State<T>& s) {
  if (!s.h_weight_stale) return NBODY_OK;
  const int64_t n = s.n;
  s.h_weight.resize((size_t)n);
  if (n) HIPCHK(c, hipMemcpyAsync(s.h_weight.data(), s.set[s.cur].weight, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  s.h_weight_stale = false;
  return NBODY_OK;
}

// A linearised tree in s.tree (the host builders', or a caller's: walk_tree) becomes the tree the walks use: its records go
// to the device and the rows into its order, as the in-place partition leaves `self.particles` (bvh_tree.rs:73-77); for the
// quad tree the leaf-ordered copies.  s.h_weight must be current (refresh_host_weights).
template <class T> int install_host_tree(nbody_ctx* c, State<T>& s, int kind) {
  const int64_t n = s.n;
  const bool bvh = kind == NBODY_TREE_BVH;
  int rc = upload_tree(c, s);
  if (rc) return rc;
  GatherArgs<T> g = row_gather_args(s, s.order_dev);
  if (!bvh) g.vel_out = nullptr, g.weight_out = nullptr, g.ids_out = nullptr;  // the leaves' copies: positions and masses
  HIPCHK(c, launch_gather<T>(c->stream, g));
  if (bvh) {  // host mirror of the row order
    s.h_tmp.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) s.h_tmp[(size_t)i] = s.h_weight[s.tree.order[(size_t)i]];
    s.h_weight.swap(s.h_tmp);
  }
  commit_tree(c, s, s.tree.kind, (int)s.tree.size(), s.tree.max_depth, c->bvh_stops, bvh, false);
  return NBODY_OK;
}

// Phase 1 of update (main.rs:398-401): snapshot + build + upward pass.  After it, for the BVH, set[cur] holds the
// permuted particles and set[1-cur].pos the pre-build snapshot (`cloned`); for the quad tree set[1-cur].pos/.mass
// hold the leaf-ordered copies the leaves own.
template <class T> int tree_build_phase(nbody_ctx* c, State<T>& s, int kind) {
  using T2 = typename State<T>::T2;
  if (kind != NBODY_TREE_BVH && kind != NBODY_TREE_QUAD) return fail(c, NBODY_ERR_INVALID, "unknown tree kind");
  const int64_t n = s.n;
  s.tree_valid = false;
  s.tree_host_stale = false;
  c->last_build_device = true;
  c->bvh_stops = 0;
  if (kind == NBODY_TREE_QUAD && n > 0 && env_int("NBODY_TREE_BUILD_HOST", 0) == 0) {
    int rc = quad_build_device<T>(c, s);
    if (rc != 1) return rc;  // 1 = the device build declined (too deep for its key / sizes): host builder below
  }
  if (kind == NBODY_TREE_BVH && n > 0 && c->params.leaf_size >= 1 && env_int("NBODY_TREE_BUILD_HOST", 0) == 0) {
    int rc = bvh_build_device<T>(c, s);
    if (rc != 1) return rc;
  }
  c->last_build_device = false;
  int rcw = refresh_host_weights<T>(c, s);  // the host builder reads the weights in the current row order
  if (rcw) return rcw;
  const bool trace = env_int("NBODY_TRACE", 0) != 0;
  double tt0 = now_s();
  s.h_pos.resize((size_t)(2 * n));
  if (n) {
    HIPCHK(c, hipMemcpyAsync(s.h_pos.data(), s.set[s.cur].pos, (size_t)n * sizeof(T2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  double tt1 = now_s();
  if (kind == NBODY_TREE_BVH) {
    if (c->params.leaf_size < 1) return fail(c, NBODY_ERR_INVALID, "leaf_size must be >= 1");
    build_bvh<T>(s.h_pos.data(), s.h_weight.data(), n, c->params.leaf_size, s.tree);
  } else {
    build_quad<T>(s.h_pos.data(), s.h_weight.data(), n, (T)c->params.quad_root_x, (T)c->params.quad_root_y,
                  (T)c->params.quad_root_h, s.tree);
  }
  double tt2 = now_s();
  if (trace) std::fprintf(stderr, "[nbody] host tree build: D2H %.3f ms, build %.3f ms (%zu nodes)\n", 1e3 * (tt1 - tt0), 1e3 * (tt2 - tt1), s.tree.size());
  if (s.tree.overflow)
    return fail(c, NBODY_ERR_DEGENERATE, "tree build exceeded the depth cap (more coincident points than a leaf holds)");
  return install_host_tree<T>(c, s, kind);
}

template int refresh_host_weights<float>(nbody_ctx*, State<float>&);
template int refresh_host_weights<double>(nbody_ctx*, State<double>&);
template int install_host_tree<float>(nbody_ctx*, State<float>&, int);
template int install_host_tree<double>(nbody_ctx*, State<double>&, int);
template int tree_build_phase<float>(nbody_ctx*, State<float>&, int);
template int tree_build_phase<double>(nbody_ctx*, State<double>&, int);
template int download_tree<float>(nbody_ctx*, State<float>&);
template int download_tree<double>(nbody_ctx*, State<double>&);

}  // namespace nbody
