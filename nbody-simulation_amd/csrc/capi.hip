// libnbody_hip — context and extern "C" surface (include/nbody_hip.h): create/destroy, parameters, upload/download,
// the kernel timer, counters and self-tests.  The steps live beside it: direct_driver.hip (direct sum), target_driver.hip (the
// sum at points that are not bodies: probes, tracers),
// tree_build_driver.hip and tree_driver.hip (Barnes-Hut builds, walks, the step driver), caller_tree.hip (trees that cross
// the C ABI), snapshot.hip (snapshots, delta snapshots, render); multi.hip fronts several devices with one handle.
//
// Host side of the drop-in for World::update (/root/reference src/main.rs:388-425).  The context owns the
// device image of `World.particles` (main.rs:37-39) as SoA arrays; every entry point is one of the three
// phases of update (build / force / integrate) or a copy in/out.  There is no CPU fallback anywhere in the
// driver: the only host computation is the tree build, which the reference also does on the host and in
// sequence (bvh_tree.rs:56-96); forces and integration always run on the GPU.
#include <algorithm>
#include <cstring>
#include <new>

#include "bvh_build.h"
#include "direct_kernels.h"
#include "driver.h"
#include "exact_sum_emulate.h"
#include "walk_split.h"

using namespace nbody;

// ------------------------------------------------------------------------------------------------ timer
hipError_t nbody_timer::begin(hipStream_t s, Pair* out) {
  if (pool.size() >= 256) {
    hipError_t e = drain();
    if (e != hipSuccess) return e;
  }
  Pair p{};
  if (!free_.empty()) {
    p = free_.back();
    free_.pop_back();
  } else {
    hipError_t e = hipEventCreate(&p.a);
    if (e != hipSuccess) return e;
    e = hipEventCreate(&p.b);
    if (e != hipSuccess) return e;
  }
  *out = p;
  return hipEventRecord(p.a, s);
}
hipError_t nbody_timer::end(hipStream_t s, const Pair& p) {
  hipError_t e = hipEventRecord(p.b, s);
  pool.push_back(p);
  return e;
}
hipError_t nbody_timer::drain() {
  for (auto& p : pool) {
    hipError_t e = hipEventSynchronize(p.b);
    if (e != hipSuccess) return e;
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, p.a, p.b);
    if (e != hipSuccess) return e;
    total_ms += ms;
    launches++;
    free_.push_back(p);
  }
  pool.clear();
  return hipSuccess;
}
nbody_timer::~nbody_timer() {
  for (auto& p : pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto& p : free_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
}

// ------------------------------------------------------------------------------------------------ context
namespace {

thread_local std::string g_create_error;

template <class T> void free_state(State<T>& s) {
  for (auto& st : s.set) { free_dev(st.pos); free_dev(st.vel); free_dev(st.weight); free_dev(st.ids); free_dev(st.mass); }
  free_dev(s.pos_next); free_dev(s.acc); free_dev(s.geom0); free_dev(s.geom1); free_dev(s.link); free_dev(s.order_dev);
  free_dev(s.node_depth); free_dev(s.node_mass); free_dev(s.node_size); free_dev(s.qb_scratch); free_dev(s.bb_scratch); free_dev(s.ws_scratch); free_dev(s.ws_terms); free_dev(s.wt_hist);
  s.node_aux_cap = 0; s.qb_scratch_bytes = 0; s.bb_scratch_bytes = 0; s.h_weight_stale = false;
  s.ws_scratch_bytes = 0; s.ws_capacity = 0; s.ws_backoff = 0; s.quad_depth_hint = 0; s.wt_hist_n = -1; s.bvh_levels_hint = 0; s.bvh_levels_stable = 0; s.ahead_total_due = false;
  s.tree_host_stale = false; s.n_nodes = 0;
  s.node_cap = 0; s.n = 0; s.tree_valid = false; s.tree.clear();
  s.h_pos.clear(); s.h_weight.clear();
  free_dev(s.classes.rank); free_dev(s.classes.pad_slots); free_dev(s.classes.tile_mass);
  s.classes = typename State<T>::MassClasses{};
}

void free_tracers(nbody_ctx* c) {
  free_dev(c->tracers.pos); free_dev(c->tracers.vel); free_dev(c->tracers.acc); free_dev(c->tracers.mark);
  c->tracers.m = 0;
}

// -------------------------------------------------------------------------------------------- upload / download
template <class T> int upload(nbody_ctx* c, int64_t n, const T* pos, const T* vel, const uint32_t* w) {
  if (!c) return NBODY_ERR_INVALID;
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!pos || !vel))) return fail(c, NBODY_ERR_INVALID, "upload: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  c->direct_graph.reset();
  free_state(c->sf);
  free_state(c->sd);
  free_tracers(c);  // a new world
  c->has_f32 = c->has_f64 = false;
  c->dl.key_next = true;  // new bodies: the next delta snapshot starts a sequence
  State<T>& s = state_of<T>(c);
  using T2 = typename State<T>::T2;
  s.n = n;
  // tree_walk_wave reads leaf particles 8 at a time: padded; a multi-device context asks for whole blocks (row_capacity)
  const size_t nn = (size_t)std::max<int64_t>(n > 0 ? n : 1, c->row_capacity) + 16;
  for (auto& st : s.set) {
    HIPCHK(c, hipMalloc((void**)&st.pos, nn * sizeof(T2)));
    HIPCHK(c, hipMalloc((void**)&st.vel, nn * sizeof(T2)));
    HIPCHK(c, hipMalloc((void**)&st.weight, nn * sizeof(uint32_t)));
    HIPCHK(c, hipMalloc((void**)&st.ids, nn * sizeof(uint32_t)));
    HIPCHK(c, hipMalloc((void**)&st.mass, nn * sizeof(T)));
  }
  HIPCHK(c, hipMalloc((void**)&s.pos_next, nn * sizeof(T2)));
  HIPCHK(c, hipMalloc((void**)&s.acc, nn * sizeof(T2)));
  HIPCHK(c, hipMalloc((void**)&s.order_dev, nn * sizeof(uint32_t)));
  s.cur = 0;
  s.h_weight.resize((size_t)n);
  std::vector<uint32_t> ids((size_t)n);
  std::vector<T> mass((size_t)n);
  bool uniform = n > 0;
  for (int64_t i = 0; i < n; ++i) {
    s.h_weight[(size_t)i] = w ? w[i] : 1u;
    uniform = uniform && s.h_weight[(size_t)i] == s.h_weight[0];
    ids[(size_t)i] = (uint32_t)i;
    mass[(size_t)i] = (T)s.h_weight[(size_t)i];  // `weight as f32`
  }
  if (n > 0) {
    auto& st = s.set[0];
    HIPCHK(c, hipMemcpyAsync(st.pos, pos, (size_t)n * sizeof(T2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.vel, vel, (size_t)n * sizeof(T2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.weight, s.h_weight.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.ids, ids.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.mass, mass.data(), (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  s.h_weight_stale = false;
  ++s.row_epoch;
  s.uniform_mass = (uniform && s.h_weight[0] > 0) ? (float)s.h_weight[0] : 0.f;
  s.sparse_base = 0.f;
  if (!uniform && n > 0) {  // one mass but for a few bodies?  (majority vote, then a count)
    uint32_t cand = 0;
    int64_t votes = 0, odd = 0;
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t wv = s.h_weight[(size_t)i];
      if (votes == 0) { cand = wv; votes = 1; }
      else votes += (wv == cand) ? 1 : -1;
    }
    for (int64_t i = 0; i < n; ++i) odd += s.h_weight[(size_t)i] != cand;
    if (cand > 0 && odd <= n / 256) s.sparse_base = (float)cand;
  }
  s.tree_valid = false;
  if (sizeof(T) == 4) c->has_f32 = true; else c->has_f64 = true;
  return NBODY_OK;
}

template <class T> int download(nbody_ctx* c, T* pos, T* vel, uint32_t* w, uint32_t* ids) {
  if (!c) return NBODY_ERR_INVALID;
  if (!has_state<T>(c)) return fail(c, NBODY_ERR_INVALID, "download: no particles of this precision uploaded");
  State<T>& s = state_of<T>(c);
  using T2 = typename State<T>::T2;
  HIPCHK(c, hipSetDevice(c->device));
  auto& st = s.set[s.cur];
  const size_t n = (size_t)s.n;
  if (n) {
    if (pos) HIPCHK(c, hipMemcpyAsync(pos, st.pos, n * sizeof(T2), hipMemcpyDeviceToHost, c->stream));
    if (vel) HIPCHK(c, hipMemcpyAsync(vel, st.vel, n * sizeof(T2), hipMemcpyDeviceToHost, c->stream));
    if (w) HIPCHK(c, hipMemcpyAsync(w, st.weight, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (ids) HIPCHK(c, hipMemcpyAsync(ids, st.ids, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NBODY_OK;
}

// ---- tracers (ctx.h, Tracers): the arguments common to nbody_tracers_upload_* and nbody_tracers_download_*
template <class T> int tracers_check(nbody_ctx* c, const char* what) {
  if (!c) return fail(nullptr, NBODY_ERR_INVALID, std::string(what) + ": the context is NULL (tracers)");
  if (c->multi) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": tracers are not available on a context made by nbody_create_multi");
  if (!has_state<T>(c))
    return fail(c, NBODY_ERR_INVALID, std::string(what) + ((c->has_f32 || c->has_f64) ? ": tracers take the precision of the uploaded particles"
                                                                                    : ": tracers need particles uploaded first"));
  return NBODY_OK;
}

template <class T> int tracers_upload(nbody_ctx* c, int64_t m, const T* pos, const T* vel) {
  using T2 = typename State<T>::T2;
  int rc = tracers_check<T>(c, "tracers_upload");
  if (rc) return rc;
  if (m < 0) return fail(c, NBODY_ERR_INVALID, "tracers_upload: m < 0 (tracers)");
  if (m > 0 && (!pos || !vel)) return fail(c, NBODY_ERR_INVALID, "tracers_upload: pos_xy or vel_xy is NULL (tracers)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_tracers(c);
  c->tdl.key_next = true;  // new tracers: their next delta snapshot starts a sequence
  if (m == 0) return NBODY_OK;
  Tracers& tr = c->tracers;
  const size_t bytes = (size_t)m * sizeof(T2);
  hipError_t e = hipMalloc(&tr.pos, bytes);
  if (e == hipSuccess) e = hipMalloc(&tr.vel, bytes);
  if (e == hipSuccess) e = hipMalloc(&tr.acc, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&tr.mark, (size_t)m);
  if (e == hipSuccess) e = hipMemcpyAsync(tr.pos, pos, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(tr.vel, vel, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free_tracers(c);
    return fail_hip(c, e, "tracers_upload");
  }
  tr.m = m;
  return NBODY_OK;
}

template <class T> int tracers_download(nbody_ctx* c, T* pos, T* vel) {
  using T2 = typename State<T>::T2;
  int rc = tracers_check<T>(c, "tracers_download");
  if (rc) return rc;
  const Tracers& tr = c->tracers;
  if (tr.m == 0) return NBODY_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)tr.m * sizeof(T2);
  if (pos) HIPCHK(c, hipMemcpyAsync(pos, tr.pos, bytes, hipMemcpyDeviceToHost, c->stream));
  if (vel) HIPCHK(c, hipMemcpyAsync(vel, tr.vel, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

}  // namespace

int nbody::fail(nbody_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg; else g_create_error = msg;
  return code;
}

// ================================================================================================ C ABI
NB_API int nbody_abi_version(void) { return NBODY_ABI_VERSION; }

NB_API int nbody_default_params(nbody_params* p) {
  if (!p) return NBODY_ERR_INVALID;
  p->theta = 50.0f;          // main.rs:35
  p->clamp = 0.001f;         // main.rs:247-248
  p->leaf_size = 64;         // bvh_tree.rs:37
  p->order = NBODY_ORDER_AS_WRITTEN;
  p->arith = NBODY_ARITH_AUTO;
  p->quad_root_x = 0.0f;
  p->quad_root_y = 0.0f;
  p->quad_root_h = 100000.0f;  // HEIGHT, main.rs:31
  return NBODY_OK;
}

NB_API int nbody_create(nbody_ctx** out, int device_id) { return nbody::ctx_create_single(out, device_id); }

int nbody::ctx_create_single(nbody_ctx** out, int device_id) {
  if (!out) return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, NBODY_ERR_NO_DEVICE,
                std::string("nbody_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                    "); this library has no CPU path");
  if (device_id < 0 || device_id >= count) return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: device_id out of range");
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device_id);
  if (e != hipSuccess) return fail_hip(nullptr, e, "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, NBODY_ERR_NO_DEVICE, std::string("nbody_create: device is ") + prop.gcnArchName +
                                                  ", kernels are built for gfx950 (MI355X) only");
  nbody_ctx* c = new (std::nothrow) nbody_ctx();
  if (!c) return fail(nullptr, NBODY_ERR_NOMEM, "nbody_create: out of host memory");
  c->device = device_id;
  nbody_default_params(&c->params);
  e = hipSetDevice(device_id);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->snap_event, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&c->stats_dev, 3 * sizeof(unsigned long long));
  if (e != hipSuccess) {
    int rc = fail_hip(nullptr, e, "nbody_create");
    delete c;
    return rc;
  }
  *out = c;
  return NBODY_OK;
}

NB_API void nbody_destroy(nbody_ctx* c) {
  if (!c) return;
  if (c->multi) { nbody::multi_destroy(c); return; }
  nbody::ctx_destroy_single(c);
}
void nbody::ctx_destroy_single(nbody_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->direct_graph.reset();
  free_state(c->sf);
  free_state(c->sd);
  free_tracers(c);
  free_dev(c->workspace);
  free_dev(c->probe_ws);
  free_dev(c->stats_dev);
  free_dev(c->frame_work);
  free_dev(c->frame_rgba);
  free_dev(c->spec_dev);
  if (c->spec_host) (void)hipHostFree(c->spec_host);
  if (c->spec_event) (void)hipEventDestroy(c->spec_event);
  c->phases.release();
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  free_snapshot(c);
  free_delta(c);
  if (c->snap_event) (void)hipEventDestroy(c->snap_event);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

NB_API const char* nbody_last_error(const nbody_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

NB_API int nbody_set_params(nbody_ctx* c, const nbody_params* p) {
  if (!c || !p) return NBODY_ERR_INVALID;
  if (p->leaf_size < 1) return fail(c, NBODY_ERR_INVALID, "set_params: leaf_size < 1");
  if (p->order != NBODY_ORDER_AS_WRITTEN && p->order != NBODY_ORDER_CONSISTENT) return fail(c, NBODY_ERR_INVALID, "set_params: bad order");
  if (p->arith < NBODY_ARITH_AUTO || p->arith > NBODY_ARITH_EXACT) return fail(c, NBODY_ERR_INVALID, "set_params: bad arith");
  c->params = *p;
  if (c->multi) return nbody::multi_set_params(c);
  return NBODY_OK;
}
NB_API int nbody_get_params(const nbody_ctx* c, nbody_params* out) {
  if (!c || !out) return NBODY_ERR_INVALID;
  *out = c->params;
  return NBODY_OK;
}

NB_API int nbody_upload_f32(nbody_ctx* c, int64_t n, const float* pos, const float* vel, const uint32_t* w) {
  if (c && c->multi) return nbody::multi_upload(c, false, n, pos, vel, w);
  return upload<float>(c, n, pos, vel, w);
}
NB_API int nbody_upload_f64(nbody_ctx* c, int64_t n, const double* pos, const double* vel, const uint32_t* w) {
  if (c && c->multi) return nbody::multi_upload(c, true, n, pos, vel, w);
  return upload<double>(c, n, pos, vel, w);
}
NB_API int nbody_download_f32(nbody_ctx* c, float* pos, float* vel, uint32_t* w, uint32_t* ids) {
  NB_VIA_PRIMARY(c, false, download<float>(p, pos, vel, w, ids));
  return download<float>(c, pos, vel, w, ids);
}
NB_API int nbody_download_f64(nbody_ctx* c, double* pos, double* vel, uint32_t* w, uint32_t* ids) {
  NB_VIA_PRIMARY(c, false, download<double>(p, pos, vel, w, ids));
  return download<double>(c, pos, vel, w, ids);
}

NB_API int64_t nbody_num_particles(const nbody_ctx* c) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) return nbody_num_particles(nbody::multi_peek(c));
  return c->has_f32 ? c->sf.n : (c->has_f64 ? c->sd.n : 0);
}

NB_API int nbody_tracers_upload_f32(nbody_ctx* c, int64_t m, const float* pos, const float* vel) { return tracers_upload<float>(c, m, pos, vel); }
NB_API int nbody_tracers_upload_f64(nbody_ctx* c, int64_t m, const double* pos, const double* vel) { return tracers_upload<double>(c, m, pos, vel); }
NB_API int nbody_tracers_download_f32(nbody_ctx* c, float* pos, float* vel) { return tracers_download<float>(c, pos, vel); }
NB_API int nbody_tracers_download_f64(nbody_ctx* c, double* pos, double* vel) { return tracers_download<double>(c, pos, vel); }
NB_API int64_t nbody_num_tracers(const nbody_ctx* c) { return c ? c->tracers.m : 0; }

NB_API int nbody_get_counting(const nbody_ctx* c, nbody_counting* out) {
  if (!c || !out) return NBODY_ERR_INVALID;
  *out = c->counting;
  return NBODY_OK;
}

NB_API int nbody_selftest_exact_sum(const float* x, int64_t n, int tile, int seq_run, float* out_sum, int64_t* out_restarts) {
  if ((!x && n > 0) || n < 0 || tile < 1 || seq_run < 1 || !out_sum) return NBODY_ERR_INVALID;
  *out_sum = xsum::emulate_fold<float>(x, n, tile, seq_run, out_restarts);
  return NBODY_OK;
}
NB_API int nbody_selftest_div_pair(int device, const float* nx, const float* ny, const float* den, int64_t n, float* qx, float* qy) {
  if (n < 0 || (n > 0 && (!nx || !ny || !den || !qx || !qy))) return NBODY_ERR_INVALID;
  if (n == 0) return NBODY_OK;
  if (hipSetDevice(device) != hipSuccess) return NBODY_ERR_NO_DEVICE;
  float* d = nullptr;
  const size_t b = (size_t)n * sizeof(float);
  if (hipMalloc((void**)&d, 5 * b) != hipSuccess) return NBODY_ERR_HIP;
  hipError_t e = hipMemcpy(d, nx, b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, ny, b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 2 * n, den, b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_div_pair_selftest(nullptr, d, d + n, d + 2 * n, n, d + 3 * n, d + 4 * n);
  if (e == hipSuccess) e = hipMemcpy(qx, d + 3 * n, b, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(qy, d + 4 * n, b, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return e == hipSuccess ? NBODY_OK : NBODY_ERR_HIP;
}
// The one-pass walk's preparation alone (launch_tree_walk_tile_prep: no walk kernel, no tree), over a history and target ids of
// the caller's.  With `keep_scratch` the scratch block lives per thread from one call to the next: the estimate scan's state
// area is zeroed when the block is allocated and never again, as ensure_walk_scratch does it for a step.  A call without it
// takes a fresh block and leaves none behind.
namespace {
struct EstimateSelftestScratch {
  char* block = nullptr;
  size_t bytes = 0;
  int device = -1;
};
thread_local EstimateSelftestScratch g_est_scratch;
constexpr int kEstFlagWords = 128;    // the block a step packs: flags + level counters (ctx.h, StepAheadRecord::build)
constexpr int kEstBigcountAt = 32;    // where this self-test puts the level counters inside it (64 of them)
}  // namespace
NB_API int nbody_selftest_walk_estimate(int device, const uint32_t* hist, int64_t hist_n, const uint32_t* ids, int64_t n, int shift, int route,
                                        int nodes, int node_count, int fallback, int bad_index, int long_nodes_at_level_end, int level_end,
                                        int node_cap, int keep_scratch, uint32_t* out_off, int32_t* out_info, int32_t* out_verdict,
                                        int32_t* out_pack, int32_t* out_flags, int32_t* out_clear, int64_t clear_words, int64_t* out_used) {
  if (!hist || !ids || !out_off || !out_info || !out_verdict || !out_pack || !out_flags || !out_clear || !out_used) return NBODY_ERR_INVALID;
  if (n < 1 || hist_n < n || hist_n > ((int64_t)1 << 22) || shift < 0 || shift > 31 || route < 0 || route > 2) return NBODY_ERR_INVALID;
  if (route == 2 && n > kWalkFusedScanMaxTargets) return NBODY_ERR_INVALID;
  if (level_end < 0 || level_end >= kBvhLevels || clear_words < kEstFlagWords || clear_words > 65536) return NBODY_ERR_INVALID;
  for (int64_t i = 0; i < n; ++i)
    if ((int64_t)ids[i] >= hist_n) return NBODY_ERR_INVALID;  // the kernels gather hist[ids[t]] unchecked
  if (hipSetDevice(device) != hipSuccess) return NBODY_ERR_NO_DEVICE;
  const WalkSplitLayout L = walk_split_layout(n);
  EstimateSelftestScratch& sc = g_est_scratch;
  const bool kept = keep_scratch != 0 && sc.block && sc.device == device && sc.bytes >= L.total;
  uint32_t *hist_d = nullptr, *ids_d = nullptr;
  int* aux = nullptr;  // verdict (2) | pack (2 + flag words + 8) | flags block and clear region (clear_words)
  const size_t pack_words = 2 + kEstFlagWords + 8;
  auto finish = [&](hipError_t e) {
    (void)hipDeviceSynchronize();
    (void)hipFree(hist_d);
    (void)hipFree(ids_d);
    (void)hipFree(aux);
    if (keep_scratch == 0 || e != hipSuccess) {  // nothing stays allocated behind a call that did not ask for it
      (void)hipFree(sc.block);
      sc = EstimateSelftestScratch{};
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? NBODY_OK : NBODY_ERR_HIP;
  };
  hipError_t e = hipSuccess;
  if (!kept) {
    (void)hipFree(sc.block);
    sc = EstimateSelftestScratch{};
    if ((e = hipMalloc((void**)&sc.block, L.total)) != hipSuccess) { sc.block = nullptr; return finish(e); }
    sc.bytes = L.total;
    sc.device = device;
    if ((e = hipMemset(sc.block + L.scan_state, 0, L.scan_state_bytes)) != hipSuccess) return finish(e);
  }
  if ((e = hipMalloc((void**)&hist_d, (size_t)hist_n * 4)) != hipSuccess) return finish(e);
  if ((e = hipMalloc((void**)&ids_d, (size_t)n * 4)) != hipSuccess) return finish(e);
  if ((e = hipMalloc((void**)&aux, (2 + pack_words + (size_t)clear_words) * sizeof(int))) != hipSuccess) return finish(e);
  int* verdict_d = aux;
  int* pack_d = aux + 2;
  int* flags_d = aux + 2 + pack_words;
  // the flags block: every word its own value, so that the packed copy is checked word by word; then the verdict's inputs
  std::vector<int32_t> block((size_t)clear_words);
  for (int64_t k = 0; k < clear_words; ++k) block[(size_t)k] = (int32_t)(0x5A000000 + k);
  for (int k = 0; k < kBvhLevels; ++k) block[(size_t)(kEstBigcountAt + k)] = 0;
  block[kBvhFallback] = fallback;
  block[kBvhNodeCount] = node_count;
  block[kBvhBadIndex] = bad_index;
  block[kBvhNodes] = nodes;
  block[(size_t)(kEstBigcountAt + level_end)] = long_nodes_at_level_end;
  std::memcpy(out_flags, block.data(), kEstFlagWords * sizeof(int32_t));
  if ((e = hipMemcpy(hist_d, hist, (size_t)hist_n * 4, hipMemcpyHostToDevice)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(ids_d, ids, (size_t)n * 4, hipMemcpyHostToDevice)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(flags_d, block.data(), (size_t)clear_words * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return finish(e);
  if ((e = hipMemset(aux, 0, (2 + pack_words) * sizeof(int))) != hipSuccess) return finish(e);
  WalkArgs<float> w{};
  w.n_tgt = n;
  TileTail tail;
  tail.flags = flags_d;
  tail.flag_words = kEstFlagWords;
  tail.bigcount = flags_d + kEstBigcountAt;
  tail.level_end = level_end;
  tail.node_cap = node_cap;
  tail.verdict = verdict_d;
  tail.pack = pack_d;
  tail.clear = flags_d;
  tail.clear_words = (int)clear_words;
  tail.info_zeroed = false;
  tail.fused_scan = route == 2;
  int64_t waves = 0;
  if ((e = launch_tree_walk_tile_prep<float>(nullptr, w, sc.block, L, ids_d, hist_d, 1, shift, &waves, route == 0 ? nullptr : &tail)) != hipSuccess)
    return finish(e);
  if ((e = hipDeviceSynchronize()) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_off, sc.block + L.off, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_info, sc.block + L.info, 8 * sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_verdict, verdict_d, 2 * sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_pack, pack_d, pack_words * sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  if ((e = hipMemcpy(out_clear, flags_d, (size_t)clear_words * sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) return finish(e);
  out_used[0] = waves - n / 64 - 4;  // the `extra` waves of the budget rule (grid = extra + n / 64 + 4)
  out_used[1] = waves;
  out_used[2] = kept ? 1 : 0;
  out_used[3] = 0;
  return finish(hipSuccess);
}
NB_API int nbody_selftest_exact_sum_chunked(const float* x, int64_t n, int chunk, float* out_sum, int64_t* out_runs_used) {
  if ((!x && n > 0) || n < 0 || chunk < 1 || !out_sum) return NBODY_ERR_INVALID;
  // segments of 8 addends per thread, as bvh_chunk_runs cuts a chunk
  *out_sum = xsum::emulate_fold_chunked2(x, n, chunk, chunk >= 8 ? 8 : 1, out_runs_used);
  return NBODY_OK;
}
NB_API int nbody_selftest_exact_sum_f64(const double* x, int64_t n, int tile, int seq_run, double* out_sum, int64_t* out_restarts) {
  if ((!x && n > 0) || n < 0 || tile < 1 || seq_run < 1 || !out_sum) return NBODY_ERR_INVALID;
  *out_sum = xsum::emulate_fold<double>(x, n, tile, seq_run, out_restarts);
  return NBODY_OK;
}
NB_API int nbody_selftest_exact_sum_f64_segmented(const double* x, int64_t n, int seg, double* out_sum, int64_t* out_runs_used) {
  if ((!x && n > 0) || n < 0 || seg < 1 || !out_sum) return NBODY_ERR_INVALID;
  *out_sum = xsum::emulate_fold_segmented(x, n, seg, out_runs_used);
  return NBODY_OK;
}
NB_API int nbody_bvh_build_restarts(const nbody_ctx* ctx) {
  if (ctx && ctx->multi) ctx = nbody::multi_peek(ctx);
  return ctx ? ctx->bvh_stops : 0;
}
NB_API int nbody_last_build_on_device(const nbody_ctx* ctx) {
  if (ctx && ctx->multi) ctx = nbody::multi_peek(ctx);
  return ctx && ctx->last_build_device ? 1 : 0;
}

NB_API int nbody_timer_create(nbody_timer** out) {
  if (!out) return NBODY_ERR_INVALID;
  *out = new (std::nothrow) nbody_timer();
  return *out ? NBODY_OK : NBODY_ERR_NOMEM;
}
NB_API void nbody_timer_destroy(nbody_timer* t) { delete t; }
NB_API int nbody_timer_read(nbody_timer* t, int reset, double* avg_ms, int64_t* launches) {
  if (!t) return NBODY_ERR_INVALID;
  hipError_t e = t->drain();
  if (e != hipSuccess) return fail_hip(nullptr, e, "timer drain");
  if (avg_ms) *avg_ms = t->launches ? t->total_ms / (double)t->launches : 0.0;
  if (launches) *launches = t->launches;
  if (reset) { t->total_ms = 0.0; t->launches = 0; }
  return NBODY_OK;
}
NB_API int nbody_set_timer(nbody_ctx* c, nbody_timer* t) {
  if (!c) return NBODY_ERR_INVALID;
  if (c->multi) nbody::multi_peek(c)->timer = t;  // the first device's kernels are the ones timed
  c->timer = t;
  return NBODY_OK;
}

NB_API void* nbody_get_stream(const nbody_ctx* c) {
  if (c && c->multi) c = nbody::multi_peek(c);
  return c ? (void*)c->stream : nullptr;
}

// ---- what multi.hip needs of this translation unit (ctx.h)
namespace nbody {
int ctx_fail(nbody_ctx* c, int code, const std::string& msg) { return fail(c, code, msg); }
int ctx_upload(nbody_ctx* c, bool f64, int64_t n, const void* pos, const void* vel, const uint32_t* w) {
  return f64 ? upload<double>(c, n, (const double*)pos, (const double*)vel, w) : upload<float>(c, n, (const float*)pos, (const float*)vel, w);
}
}  // namespace nbody
