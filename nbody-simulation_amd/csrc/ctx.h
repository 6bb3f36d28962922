// Internal: the context of libnbody_hip and the functions its translation units share (the driver: one device;
// multi.hip: several devices behind the same handle).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "common.h"
#include "env.h"
#include "tree_build.hpp"

namespace nbody {

struct Multi;  // multi.hip: the devices of a context made by nbody_create_multi

template <class T> struct State {
  using T2 = typename Vec2T<T>::type;
  struct Set {
    T2* pos = nullptr;
    T2* vel = nullptr;
    uint32_t* weight = nullptr;
    uint32_t* ids = nullptr;
    T* mass = nullptr;
  };
  int64_t n = 0;
  Set set[2];
  int cur = 0;
  T2* pos_next = nullptr;  // direct step output, swapped with set[cur].pos
  float uniform_mass = 0.f;  // > 0 when every weight is the same value (checked on upload)
  float sparse_base = 0.f;   // > 0 when every weight is this value but for at most n/256 bodies (the reference's scene)
  // Mass classes (direct step, masses that differ freely but take at most 32 values): the far copy of the positions is
  // written in class order, every class padded to whole 1024-source tiles, so the main pass runs the equal-mass arithmetic
  // tile by tile.  Built lazily for the current row order (row_epoch moves whenever a build permutes the rows).
  struct MassClasses {
    uint64_t epoch = ~0ull;        // row_epoch these arrays were built for
    bool usable = false;           // 2 .. 32 distinct masses, none of the cheaper cases
    int n_classes = 0;
    int64_t n_slots = 0;           // bodies + padding
    int n_pad_slots = 0;
    uint32_t* rank = nullptr;      // [n] device: body -> slot
    uint32_t* pad_slots = nullptr; // [n_pad_slots] device
    float* tile_mass = nullptr;    // [n_slots / 1024] device
  } classes;
  uint64_t row_epoch = 0;
  T2* acc = nullptr;
  // tree
  void* geom0 = nullptr;
  void* geom1 = nullptr;
  void* link = nullptr;
  size_t node_cap = 0;
  uint32_t* order_dev = nullptr;
  TreeHost<T> tree;          // host image of the last build (filled lazily after a device build)
  bool tree_valid = false;
  bool tree_host_stale = false;  // the last build ran on the device and has not been downloaded
  int n_nodes = 0, tree_kind = 0, tree_max_depth = 0;
  int shard_kind = 0;            // tree kind of the last sharded step (decides how a slice maps to rows)
  int* node_depth = nullptr;     // device build: depth of every node
  uint32_t* node_mass = nullptr; // device build: u32 mass of every node
  T2* node_size = nullptr;       // device BVH build: boundary.size of every node
  size_t node_aux_cap = 0;
  char* qb_scratch = nullptr;
  size_t qb_scratch_bytes = 0;
  char* bb_scratch = nullptr;    // device BVH build
  size_t bb_scratch_bytes = 0;
  bool h_weight_stale = false;   // a device BVH build permuted the rows without touching h_weight (row_epoch moves with it)
  int quad_depth_hint = 0;       // depth of the last device-built quad tree (how many levels the next build sorts by)
  int bvh_levels_hint = 0;       // long-node levels the last device-built BVH had (how many the next step enqueues blind)
  int bvh_levels_stable = 0;     // consecutive step-ahead builds that had exactly that many: after eight the spare blind level is dropped
  bool bb_flags_clean = false;   // the BVH build's flags and level counters are zero (the step enqueued ahead left them so)
  bool ahead_total_due = false;  // the last ahead-step's exact term count has not been read back yet
  // split walk (walk_prepare.hip, walk_lab.hip): counts/offsets scratch and the term array
  char* ws_scratch = nullptr;
  size_t ws_scratch_bytes = 0;
  void* ws_terms = nullptr;
  int64_t ws_capacity = 0;       // terms
  int ws_backoff = 0;            // steps for which the split walk is not tried (the last one needed too much memory)
  // one-pass walk (walk_tile): the counts in ws_scratch are those of the last walk over the context's own particles
  int64_t wt_hist_n = -1, wt_hist_begin = 0;
  unsigned long long wt_total = 0;  // terms of that walk
  uint32_t* wt_hist = nullptr;      // [n] per particle id: its terms in that walk
  std::vector<T> h_pos;
  std::vector<uint32_t> h_weight;  // current row order
  std::vector<uint32_t> h_tmp;
};


// Massless tracers that step with the bodies (target_kernels.h; nbody_tracers_*): rows of the context's precision in upload order,
// for ever — the BVH's permutations concern bodies only.  `acc` receives a tree step's walk at the tracers; `mark` a direct step's
// decision per tracer (1: EXACT), taken from the pre-step positions before anything is integrated.
struct Tracers {
  int64_t m = 0;
  void* pos = nullptr;
  void* vel = nullptr;
  void* acc = nullptr;
  uint8_t* mark = nullptr;
};

// One sequence of delta snapshots (delta_snapshot.hip): three key arrays in rotation (this / previous / the one before), the pieces
// of the stream on the device, the assembled stream in pinned memory.
struct DeltaStream {
  void* keys[3] = {nullptr, nullptr, nullptr};
  int cur = 0;
  uint8_t* widths = nullptr;
  uint32_t *words = nullptr, *offsets = nullptr;
  void* scan = nullptr;
  size_t scan_bytes = 0;
  uint64_t *payload = nullptr, *total = nullptr, *htotal = nullptr;
  uint8_t* host = nullptr;
  int64_t n = -1;  // elements the buffers are sized for
  int bits = 0;
  bool key_next = true, pending = false;
  size_t stream_bytes = 0;
  uint64_t step = 0;
};

// The `uniform_mass` argument of the direct step for this state: > 0 all equal, < 0 all equal to its magnitude but a few, 0 neither.
template <class T> inline float direct_mass_hint(const State<T>& s) { return s.uniform_mass > 0.f ? s.uniform_mass : -s.sparse_base; }

// A direct step as ctx_direct_prep sees it, and what one ctx_direct_run over a block of its targets adds.  `n_tgt_total`: all targets this
// device computes in the step (decides whether the near/far split pays); `n_tgt_max`: the largest block of one run (sizes the workspace).
struct DirectStep {
  hipStream_t stream = nullptr;
  int64_t n_src = 0;
  const void *pos_all = nullptr, *mass_all = nullptr;
  float uniform_mass = 0.f, clamp = 0.f;  // (uniform_mass: direct_mass_hint())
  int arith = 0;
  int64_t n_tgt_total = 0, n_tgt_max = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
};
struct DirectBlock {
  int64_t tgt_begin = 0, n_tgt = 0;
  void *vel = nullptr, *pos_out = nullptr, *acc_out = nullptr;  // rows of the block's first target
  float delta = 0.f;
  nbody_timer* timer = nullptr;
};

// Two consecutive direct steps (A -> B -> A position buffers) captured once as a hipGraph and replayed: a small-N step
// is ~15 launches (hazard scan, near/far split, gated kernels), i.e. launch-bound (N = 1024: 78 us per eager step
// against 13 us of kernels).  The graph is rebuilt when anything it baked in changes: its key.
struct DirectGraphKey {
  int64_t n = -1;
  const void *pos_a = nullptr, *pos_b = nullptr, *vel = nullptr, *mass = nullptr, *ws = nullptr;
  float delta = 0.f, clamp = 0.f, uniform = 0.f;
  int arith = -1;
  // what the step derives from the row order: the mass classes' arrays (their addresses are kernel arguments of the capture)
  uint64_t row_epoch = ~0ull;
  bool cls_usable = false;
  const void *cls_rank = nullptr, *cls_tile_mass = nullptr;
  std::string env;  // the NBODY_DIRECT_* switches read at capture time
  auto tied() const { return std::tie(n, pos_a, pos_b, vel, mass, ws, delta, clamp, uniform, arith, row_epoch, cls_usable, cls_rank, cls_tile_mass, env); }
  bool operator==(const DirectGraphKey& o) const { return tied() == o.tied(); }
};
struct DirectGraph {
  hipGraphExec_t exec = nullptr;
  DirectGraphKey key;
  void reset() {
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
    key = DirectGraphKey{};
  }
};
inline std::string direct_env_signature() {
  std::string sig;
  const char* nf = getenv("NBODY_DIRECT_NEARFAR");
  sig += nf ? nf : "-";
  sig += ';';
  for (const char* k : {"NBODY_DIRECT_ASM", "NBODY_DIRECT_TPT", "NBODY_DIRECT_GSPLIT", "NBODY_DIRECT_NO_UNIFORM", "NBODY_DIRECT_NO_CLASSES",
                        "NBODY_DIRECT_NO_SPARSE",
                        "NBODY_DIRECT_MUTUAL_MIN_N"}) {  // (laboratory build only)
    const char* v = lab_str(k);
    sig += v ? v : "-";
    sig += ';';
  }
  return sig;
}

// The three phases of a tree step (Counting, main.rs:74-79) timed by four events on the step's stream: the stream idles
// while the host works inside a phase (a host-side build), so device-timeline intervals cover host time too, and no
// phase boundary needs a host synchronisation.
struct PhaseEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool borrowed = false;  // e[0] is the previous step's e[3]
};
// What the context keeps of its steps' phase timing (phase_clock.h: StepClock, phase_drain).  The steps enqueued ahead
// (tree_driver.hip, bvh_step_ahead) are timed by their own kernels instead of three event records per step (each ~6 us of idle
// stream): the kernels write the 100 MHz wall clock at the phase boundaries, slot = {build begins, walk begins, integration
// begins, step ends}; read back when the phases are drained.
struct PhaseTiming {
  unsigned long long* stamp_dev = nullptr;  // [kStampSlots][4]
  std::vector<int> stamp_pending;           // slots of finished steps not yet read
  int stamp_next = 0;
  int stamp_open = -1;                      // slot whose end is still to be written (by the next step's first kernel, or a stamp kernel)
  std::vector<PhaseEvents> pending;         // recorded phase events
  std::vector<hipEvent_t> free_events;      // reusable events
  nbody_counting* counter = nullptr;        // the caller's counter of the call in progress
  void release() {                          // (the context is being destroyed)
    if (stamp_dev) (void)hipFree(stamp_dev);
    for (auto& p : pending)
      for (int k = p.borrowed ? 1 : 0; k < 4; ++k)
        if (p.e[k]) (void)hipEventDestroy(p.e[k]);
    for (auto e : free_events) (void)hipEventDestroy(e);
  }
};
// The pinned record a BVH step enqueued ahead of the host packs for it (tree_driver.hip, bvh_step_ahead).  The device side sees
// plain words: TileTail::pack writes verdict | build | info_before in one run, the integration's Gate carries info_after.
struct StepAheadRecord {
  int verdict[2];       // node count or 0, ok
  int build[128];       // the build's flags, and its level counters where the build's layout has them (512 B)
  int info_before[8];   // the walk's info once its preparation is done
  int info_after[8];    // ... and after the walk (its exact term count), read one step late
};
static_assert(sizeof(StepAheadRecord) == (2 + 128 + 8 + 8) * sizeof(int), "the record's parts lie back to back");
constexpr int kAheadBuildWords = sizeof(StepAheadRecord::build) / sizeof(int);
}  // namespace nbody

struct nbody_ctx {
  nbody::Multi* multi = nullptr;   // non-null: this handle fronts several devices (multi.hip) and owns no device state itself
  int64_t row_capacity = 0;        // rows the particle arrays are allocated for (>= n; a multi context pads to its block layout)
  nbody::DirectGraph direct_graph;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  nbody_params params{};
  nbody_counting counting{};
  nbody_timer* timer = nullptr;
  bool has_f32 = false, has_f64 = false;
  nbody::State<float> sf;
  nbody::State<double> sd;
  void* workspace = nullptr;
  int bvh_stops = 0;  // exact-sum restarts of the last device BVH build (diagnostic)
  bool last_build_device = false;
  size_t workspace_bytes = 0;
  unsigned long long* stats_dev = nullptr;
  uint32_t* frame_work = nullptr;  // render: per-pixel counters
  hipStream_t copy_stream = nullptr;  // snapshot transfers, concurrent with the steps on `stream`
  hipEvent_t snap_event = nullptr;
  bool snap_pending = false;
  uint64_t steps_done = 0, snap_step = 0;
  // snapshot staging: device copy of the rows, pinned host image
  void *snap_pos = nullptr, *snap_vel = nullptr, *snap_hpos = nullptr, *snap_hvel = nullptr;
  uint32_t *snap_w = nullptr, *snap_ids = nullptr, *snap_hw = nullptr, *snap_hids = nullptr;
  size_t snap_bytes2 = 0;  // bytes of one position array the staging holds
  int64_t snap_n = 0;
  bool snap_f64 = false;
  // ... and of the tracers the context held at begin (nbody_snapshot_tracers_*); the staging grows with m
  void *snap_tpos = nullptr, *snap_tvel = nullptr, *snap_htpos = nullptr, *snap_htvel = nullptr;
  size_t snap_tcap = 0;    // bytes each of the four holds
  int64_t snap_m = 0;      // tracers of the pending snapshot
  nbody::DeltaStream dl;   // delta snapshots of the bodies' positions, in id order
  nbody::DeltaStream tdl;  // ... and of the tracers', in upload order: a sequence of its own (nbody_tracers_delta_*)
  uint8_t* frame_rgba = nullptr;
  uint32_t frame_px = 0;
  unsigned long long last_stats[3] = {0, 0, 0};
  bool want_stats = false;
  nbody::PhaseTiming phases;  // the tree steps' phase clock
  // a BVH step enqueued whole, ahead of the host's knowledge of its build (tree_driver.hip, bvh_step_ahead)
  int* spec_dev = nullptr;    // [2] verdict of the build: node count or 0, ok
  nbody::StepAheadRecord* spec_host_dev = nullptr;  // spec_host as the device addresses it (kernels write the record there themselves)
  nbody::StepAheadRecord* spec_host = nullptr;      // pinned
  hipEvent_t spec_event = nullptr;
  // the direct sum at arbitrary points and the tracers' share of a direct step (target_driver.hip): flag word, a batch of targets and results, the FAST partial sums
  void* probe_ws = nullptr;
  size_t probe_ws_bytes = 0;
  nbody::Tracers tracers;  // of the precision of the bodies; a body upload removes them
};

namespace nbody {
// ---- the single-device driver: capi.hip (context, upload), tree_driver.hip (tree steps), direct_driver.hip (direct steps), target_driver.hip (probes, tracers)
int ctx_fail(nbody_ctx* c, int code, const std::string& msg);  // c == NULL: the thread's create error
int ctx_create_single(nbody_ctx** out, int device_id);
void ctx_destroy_single(nbody_ctx* c);
int ctx_upload(nbody_ctx* c, bool f64, int64_t n, const void* pos, const void* vel, const uint32_t* w);
int ctx_update_tree(nbody_ctx* c, bool f64, int kind, double delta, int n_steps, nbody_counting* counter);  // the single-device call
int ctx_update_tree_shard(nbody_ctx* c, bool f64, int kind, double delta, int64_t begin, int64_t count, nbody_counting* counter);
int ctx_export_slice(nbody_ctx* c, int64_t begin, int64_t count, void* rows, void* pos, void* vel);
int ctx_import_rows(nbody_ctx* c, int64_t n_rows, const void* rows, const void* pos, const void* vel);
size_t ctx_direct_ws_bytes(int64_t n_src, int64_t n_tgt);
int ctx_ensure_workspace(nbody_ctx* c, size_t bytes);
int ctx_ensure_mass_classes(nbody_ctx* c);  // State::MassClasses of the f32 rows, for the direct steps that follow
int ctx_direct_prep(nbody_ctx* c, const DirectStep& step);  // decides, on the stream, which kernels of this step do the work
int ctx_direct_run(nbody_ctx* c, const DirectStep& step, const DirectBlock& block);  // force + integration of one block under that decision
// nbody_accel_direct_at_* on one device, arguments checked, n_targets > 0 (target_driver.hip)
int ctx_accel_direct_at(nbody_ctx* c, bool f64, int64_t n_targets, const void* target_xy, void* acc_xy);
// ---- multi.hip (`front` is the handle nbody_create_multi returned)
void multi_destroy(nbody_ctx* front);
int multi_set_params(nbody_ctx* front);
int multi_upload(nbody_ctx* front, bool f64, int64_t n, const void* pos, const void* vel, const uint32_t* w);
nbody_ctx* multi_peek(const nbody_ctx* front);            // the first device's context, as it is
int multi_primary(nbody_ctx* front, nbody_ctx** out);     // ... after bringing every replica up to date
int multi_replicate(nbody_ctx* front);                    // the first device's rows to every other replica
int multi_update_direct(nbody_ctx* front, float delta, int n_steps, nbody_counting* counter);
int multi_accel_direct_at(nbody_ctx* front, bool f64, int64_t n_targets, const void* target_xy, void* acc_xy);  // a block of targets per device
int multi_update_tree(nbody_ctx* front, bool f64, int kind, double delta, int n_steps, nbody_counting* counter);
}  // namespace nbody
