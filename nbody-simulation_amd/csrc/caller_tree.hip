// libnbody_hip — trees that cross the C ABI: a caller's linearised tree checked (tree_shape_ok) and walked
// (nbody_walk_tree_*, nbody_tree_validate), the context's last tree exported (nbody_tree_info, nbody_tree_export_*), and
// trees built on the host alone, without a context (nbody_host_tree_*).
#include <cstring>
#include <new>
#include <vector>

#include "driver.h"
#include "tree_build.hpp"

using namespace nbody;

struct nbody_host_tree {
  bool is_f64 = false;
  TreeHost<float> tf;
  TreeHost<double> td;
};

namespace {

// ---- a caller's tree (the force map alone, main.rs:406-416, for a host that keeps bvh_tree.rs:56-158) --------
// What the walks rely on and a foreign tree has to prove before it reaches the device: every skip link points forward (the
// walk's node index only ever grows: it ends), subtrees nest, an inner node's children are i + 1, skip[i + 1], ... and its range is
// their ranges one after the other (the walks take the range of an inner node whose children are two leaves in one step),
// leaves are single nodes, every range lies inside the particles, `order` is a permutation.  BVH: two children (BVHTree::Root,
// bvh_tree.rs:28); quad: one to four (quad_tree.rs:47-50).  The geometry and the masses are only ever operands.
bool tree_shape_ok(int kind, int64_t m, const int32_t* is_leaf, const int64_t* first, const int64_t* count, const int64_t* skip,
                   int64_t n, const uint32_t* order, int* max_depth, std::string& why) {
  auto bad = [&](int64_t i, const char* what) {
    why = "node " + std::to_string(i) + ": " + what;
    return false;
  };
  if (kind != NBODY_TREE_BVH && kind != NBODY_TREE_QUAD) { why = "unknown tree kind"; return false; }
  if (m < 1 || m > (int64_t)INT32_MAX - 1) { why = "n_nodes out of range"; return false; }
  if (n < 0 || n > (int64_t)INT32_MAX - 64) { why = "particle count out of range"; return false; }
  if (!is_leaf || !first || !count || !skip || (n > 0 && !order)) { why = "a tree array is NULL"; return false; }
  const int max_kids = kind == NBODY_TREE_BVH ? 2 : 4, min_kids = kind == NBODY_TREE_BVH ? 2 : 1;
  struct Open { int64_t id, end, cursor; int kids; };
  std::vector<Open> open;
  int deepest = 0;
  auto close = [&](const Open& o) {
    if (o.cursor != first[o.id] + count[o.id]) return bad(o.id, "its range is not its children's ranges one after the other");
    if (o.kids < min_kids || o.kids > max_kids) return bad(o.id, kind == NBODY_TREE_BVH ? "a BVH root has two children" : "a quad root has one to four children");
    return true;
  };
  for (int64_t i = 0; i < m; ++i) {
    while (!open.empty() && open.back().end == i) {
      if (!close(open.back())) return false;
      open.pop_back();
    }
    if (i > 0 && open.empty()) return bad(i, "lies outside the root's subtree (skip[0] must be n_nodes)");
    if (skip[i] <= i || skip[i] > m) return bad(i, "skip does not point forward inside the tree");
    if (first[i] < 0 || count[i] < 0 || first[i] > n || count[i] > n - first[i]) return bad(i, "range outside the particles");
    if (!open.empty()) {
      Open& parent = open.back();
      if (skip[i] > parent.end) return bad(i, "subtree reaches past its parent's");
      if (first[i] != parent.cursor) return bad(i, "range does not follow its sibling's");
      parent.cursor += count[i];
      ++parent.kids;
    }
    if (is_leaf[i]) {
      if (skip[i] != i + 1) return bad(i, "a leaf with nodes below it");
    } else {
      if (skip[i] == i + 1) return bad(i, "a root without children");
      open.push_back({i, skip[i], first[i], 0});
      if ((int)open.size() > deepest) deepest = (int)open.size();
    }
  }
  while (!open.empty()) {
    if (open.back().end != m) return bad(open.back().id, "subtree ends past the last node");
    if (!close(open.back())) return false;
    open.pop_back();
  }
  if (skip[0] != m) return bad(0, "skip[0] must be n_nodes");
  if (first[0] != 0 || count[0] != n) return bad(0, "the root's range must be every particle");
  std::vector<bool> seen((size_t)n, false);
  for (int64_t k = 0; k < n; ++k) {
    if (order[k] >= (uint64_t)n || seen[order[k]]) { why = "order is not a permutation of the rows"; return false; }
    seen[order[k]] = true;
  }
  if (max_depth) *max_depth = deepest;
  return true;
}

template <class T>
int walk_tree(nbody_ctx* c, int kind, int64_t m, const T* geom, const uint32_t* mass, const int32_t* is_leaf, const int64_t* first,
              const int64_t* count, const int64_t* skip, const uint32_t* order, int64_t n_targets, const T* target_xy, T* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "walk_tree: no particles of this precision uploaded");
  if (!geom || !mass) return fail(c, NBODY_ERR_INVALID, "walk_tree: geom or mass is NULL");
  if (!acc_xy) return fail(c, NBODY_ERR_INVALID, "walk_tree: acc_xy is NULL");
  if (target_xy && n_targets < 0) return fail(c, NBODY_ERR_INVALID, "walk_tree: n_targets < 0");
  State<T>& s = state_of<T>(c);
  std::string why;
  int depth = 0;
  if (!tree_shape_ok(kind, m, is_leaf, first, count, skip, s.n, order, &depth, why)) return fail(c, NBODY_ERR_INVALID, "walk_tree: " + why);
  HIPCHK(c, hipSetDevice(c->device));
  int rc = refresh_host_weights<T>(c, s);
  if (rc) return rc;
  s.tree_valid = false;
  s.tree_host_stale = false;
  c->last_build_device = false;
  c->bvh_stops = 0;
  TreeHost<T>& t = s.tree;
  t.clear();
  t.kind = kind;
  t.max_depth = depth;
  t.geom0.resize((size_t)m); t.geom1.resize((size_t)m); t.link.resize((size_t)m);
  t.size_x.resize((size_t)m); t.size_y.resize((size_t)m); t.mass_u32.resize((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const size_t k = (size_t)i;
    if (kind == NBODY_TREE_BVH) {
      const T* g = geom + 6 * k;
      const T w = g[2], h = g[3];
      const T tx = sse_max(w, h), ty = sse_max(h, w);  // size.max(size.yx()), main.rs:371 (as build_bvh and bvh_emit)
      t.geom0[k] = {g[0], g[1], g[0] + w, g[1] + h};
      t.geom1[k] = {g[4], g[5], (T)mass[k], tx * ty};
      t.size_x[k] = w; t.size_y[k] = h;
    } else {
      const T* g = geom + 5 * k;
      const T h = g[2];
      t.geom0[k] = {g[0], g[1], g[0] + h, g[1] + h};
      t.geom1[k] = {g[3], g[4], (T)mass[k], h * h};
      t.size_x[k] = h; t.size_y[k] = h;
    }
    t.mass_u32[k] = mass[k];
    t.link[k] = {(int32_t)skip[k], (int32_t)first[k], (int32_t)count[k], is_leaf[k] ? 1 : 0};
  }
  t.order.assign(order, order + s.n);
  rc = install_host_tree<T>(c, s, kind);
  if (rc) return rc;
  return accel_built_tree<T>(c, s, kind, n_targets, target_xy, acc_xy);
}

template <class T>
void tree_export_host(const TreeHost<T>& t, T* geom, uint32_t* mass, int32_t* is_leaf, int64_t* first, int64_t* count,
                      int64_t* skip, uint32_t* order) {
  const size_t m = t.size();
  for (size_t i = 0; i < m; ++i) {
    if (geom) {
      if (t.kind == NBODY_TREE_BVH) {
        T* g = geom + 6 * i;
        g[0] = t.geom0[i].a; g[1] = t.geom0[i].b; g[2] = t.size_x[i]; g[3] = t.size_y[i];
        g[4] = t.geom1[i].a; g[5] = t.geom1[i].b;
      } else {
        T* g = geom + 5 * i;
        g[0] = t.geom0[i].a; g[1] = t.geom0[i].b; g[2] = t.size_x[i]; g[3] = t.geom1[i].a; g[4] = t.geom1[i].b;
      }
    }
    if (mass) mass[i] = t.mass_u32[i];
    if (is_leaf) is_leaf[i] = t.link[i].is_leaf;
    if (first) first[i] = t.link[i].first;
    if (count) count[i] = t.link[i].count;
    if (skip) skip[i] = t.link[i].skip;
  }
  if (order && !t.order.empty()) std::memcpy(order, t.order.data(), t.order.size() * sizeof(uint32_t));
}

template <class T>
int tree_export(const nbody_ctx* cc, T* geom, uint32_t* mass, int32_t* is_leaf, int64_t* first, int64_t* count,
                int64_t* skip, uint32_t* order) {
  nbody_ctx* c = const_cast<nbody_ctx*>(cc);
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "tree_export: no particles of this precision uploaded");
  State<T>& s = state_of<T>(c);
  if (!s.tree_valid) return fail(c, NBODY_ERR_INVALID, "tree_export: no tree built yet");
  int rc = download_tree<T>(c, s);
  if (rc) return rc;
  tree_export_host<T>(s.tree, geom, mass, is_leaf, first, count, skip, order);
  return NBODY_OK;
}

}  // namespace

NB_API int nbody_walk_tree_f32(nbody_ctx* c, int kind, int64_t n_nodes, const float* geom, const uint32_t* mass, const int32_t* is_leaf,
                               const int64_t* leaf_first, const int64_t* leaf_count, const int64_t* skip, const uint32_t* order,
                               int64_t n_targets, const float* target_xy, float* acc_xy) {
  NB_VIA_PRIMARY(c, true, walk_tree<float>(p, kind, n_nodes, geom, mass, is_leaf, leaf_first, leaf_count, skip, order, n_targets, target_xy, acc_xy));
  return walk_tree<float>(c, kind, n_nodes, geom, mass, is_leaf, leaf_first, leaf_count, skip, order, n_targets, target_xy, acc_xy);
}
NB_API int nbody_walk_tree_f64(nbody_ctx* c, int kind, int64_t n_nodes, const double* geom, const uint32_t* mass, const int32_t* is_leaf,
                               const int64_t* leaf_first, const int64_t* leaf_count, const int64_t* skip, const uint32_t* order,
                               int64_t n_targets, const double* target_xy, double* acc_xy) {
  NB_VIA_PRIMARY(c, true, walk_tree<double>(p, kind, n_nodes, geom, mass, is_leaf, leaf_first, leaf_count, skip, order, n_targets, target_xy, acc_xy));
  return walk_tree<double>(c, kind, n_nodes, geom, mass, is_leaf, leaf_first, leaf_count, skip, order, n_targets, target_xy, acc_xy);
}
NB_API int nbody_tree_validate(int kind, int64_t n_nodes, const int32_t* is_leaf, const int64_t* leaf_first, const int64_t* leaf_count,
                               const int64_t* skip, int64_t n_particles, const uint32_t* order, char* reason, size_t reason_cap) {
  std::string why;
  const bool ok = tree_shape_ok(kind, n_nodes, is_leaf, leaf_first, leaf_count, skip, n_particles, order, nullptr, why);
  if (reason && reason_cap) {
    const size_t k = why.size() < reason_cap - 1 ? why.size() : reason_cap - 1;
    std::memcpy(reason, why.data(), k);
    reason[k] = 0;
  }
  return ok ? NBODY_OK : NBODY_ERR_INVALID;
}

NB_API int nbody_tree_info(const nbody_ctx* c, nbody_tree_view* out) {
  if (!c || !out) return NBODY_ERR_INVALID;
  if (c->multi) return nbody_tree_info(nbody::multi_peek(c), out);
  auto view = [out](const auto& s) { out->n_nodes = s.n_nodes; out->kind = s.tree_kind; out->max_depth = s.tree_max_depth; return NBODY_OK; };
  if (c->has_f32 && c->sf.tree_valid) return view(c->sf);
  if (c->has_f64 && c->sd.tree_valid) return view(c->sd);
  return fail(const_cast<nbody_ctx*>(c), NBODY_ERR_INVALID, "tree_info: no tree built yet");
}
NB_API int nbody_tree_export_f32(const nbody_ctx* c, float* geom, uint32_t* mass, int32_t* is_leaf, int64_t* first,
                                 int64_t* count, int64_t* skip, uint32_t* order) {
  if (c && c->multi) c = nbody::multi_peek(c);
  return tree_export<float>(c, geom, mass, is_leaf, first, count, skip, order);
}
NB_API int nbody_tree_export_f64(const nbody_ctx* c, double* geom, uint32_t* mass, int32_t* is_leaf, int64_t* first,
                                 int64_t* count, int64_t* skip, uint32_t* order) {
  if (c && c->multi) c = nbody::multi_peek(c);
  return tree_export<double>(c, geom, mass, is_leaf, first, count, skip, order);
}
template <class T>
static int host_tree_build(int kind, int64_t n, const T* pos, const uint32_t* w, const nbody_params* p, nbody_host_tree** out) {
  if (!out) return fail(nullptr, NBODY_ERR_INVALID, "host_tree_build: out is NULL");
  *out = nullptr;
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && !pos)) return fail(nullptr, NBODY_ERR_INVALID, "host_tree_build: bad arguments");
  nbody_params dflt;
  nbody_default_params(&dflt);
  if (!p) p = &dflt;
  if (p->leaf_size < 1) return fail(nullptr, NBODY_ERR_INVALID, "host_tree_build: leaf_size < 1");
  auto* h = new (std::nothrow) nbody_host_tree();
  if (!h) return fail(nullptr, NBODY_ERR_NOMEM, "host_tree_build: out of memory");
  TreeHost<T>* t;
  if constexpr (sizeof(T) == 8) { h->is_f64 = true; t = &h->td; } else { t = &h->tf; }
  if (kind == NBODY_TREE_BVH) build_bvh<T>(pos, w, n, p->leaf_size, *t);
  else if (kind == NBODY_TREE_QUAD) build_quad<T>(pos, w, n, (T)p->quad_root_x, (T)p->quad_root_y, (T)p->quad_root_h, *t);
  else { delete h; return fail(nullptr, NBODY_ERR_INVALID, "host_tree_build: unknown tree kind"); }
  *out = h;
  return t->overflow ? NBODY_ERR_DEGENERATE : NBODY_OK;
}

NB_API int nbody_host_tree_build_f32(int kind, int64_t n, const float* pos_xy, const uint32_t* weight,
                                     const nbody_params* p, nbody_host_tree** out) {
  return host_tree_build<float>(kind, n, pos_xy, weight, p, out);
}
NB_API int nbody_host_tree_build_f64(int kind, int64_t n, const double* pos_xy, const uint32_t* weight,
                                     const nbody_params* p, nbody_host_tree** out) {
  return host_tree_build<double>(kind, n, pos_xy, weight, p, out);
}
NB_API void nbody_host_tree_free(nbody_host_tree* t) { delete t; }
NB_API int nbody_host_tree_info(const nbody_host_tree* t, nbody_tree_view* out) {
  if (!t || !out) return NBODY_ERR_INVALID;
  if (t->is_f64) { out->n_nodes = (int64_t)t->td.size(); out->kind = t->td.kind; out->max_depth = t->td.max_depth; }
  else { out->n_nodes = (int64_t)t->tf.size(); out->kind = t->tf.kind; out->max_depth = t->tf.max_depth; }
  return NBODY_OK;
}
NB_API int nbody_host_tree_export_f32(const nbody_host_tree* t, float* geom, uint32_t* mass, int32_t* is_leaf,
                                      int64_t* first, int64_t* count, int64_t* skip, uint32_t* order) {
  if (!t || t->is_f64) return fail(nullptr, NBODY_ERR_INVALID, "host_tree_export_f32: not an f32 tree");
  tree_export_host<float>(t->tf, geom, mass, is_leaf, first, count, skip, order);
  return NBODY_OK;
}
NB_API int nbody_host_tree_export_f64(const nbody_host_tree* t, double* geom, uint32_t* mass, int32_t* is_leaf,
                                      int64_t* first, int64_t* count, int64_t* skip, uint32_t* order) {
  if (!t || !t->is_f64) return fail(nullptr, NBODY_ERR_INVALID, "host_tree_export_f64: not an f64 tree");
  tree_export_host<double>(t->td, geom, mass, is_leaf, first, count, skip, order);
  return NBODY_OK;
}
