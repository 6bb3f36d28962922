/*
 * nbody_hip.h — C ABI of the MI355X (gfx950) n-body force + integration step.
 *
 * Drop-in boundary for the hot path of KristinnVikarJ/nbody-simulation.  The reference has no FFI of its
 * own (no `extern`, `#[no_mangle]`, `repr(C)` anywhere); the seam this library replaces is the single call
 *
 *     world.update(STEP_SIZE, &mut counter)            src/main.rs:120  ->  World::update  src/main.rs:388-425
 *
 * and its three inner phases: tree build + upward pass (main.rs:400-401, bvh_tree.rs:56-158), force map
 * (main.rs:406-416 -> bvh_sum_gravity :348-386 -> calculate_gravity :234-253) and the semi-implicit Euler
 * loop (main.rs:419-423).  `Particle` (main.rs:193-198) is not repr(C), so the ABI takes separate flat
 * arrays: pos_xy / vel_xy interleaved (x0,y0,x1,y1,...) and weight as u32, caller-owned, copied in/out.
 *
 * Conventions
 *   - Every function returns 0 (NBODY_OK) or a negative nbody_status; nothing aborts or unwinds.
 *     nbody_last_error() gives the message of the last failure on that context (or, with ctx == NULL,
 *     of the last failed nbody_create on this thread).
 *   - A context belongs to one host thread at a time (the reference calls update from one dedicated
 *     thread only, main.rs:110-141).  Calls are synchronous unless the name ends in _dev (those enqueue
 *     on the given hipStream_t and return).
 *   - nbody_create: one context = one GPU.  nbody_create_multi: one context = several GPUs of one node; every
 *     nbody_update_* on it shards the step's targets over them and does the step's one exchange (an all-gather
 *     over xGMI, RCCL) inside the library, so the host keeps its single `world.update` call (main.rs:120).
 *     A host that runs one process per GPU instead uses the *_dev / *_shard calls and its own collective.
 *   - There is no CPU fallback: without a gfx950 device nbody_create fails with NBODY_ERR_NO_DEVICE.
 *
 * Environment.  libnbody_hip.so reads these nine variables and no others (tests/test_capi_host.py checks the binary against
 * this list); results are the same bits whatever they are set to — they choose between equivalent ways of getting them:
 *   NBODY_TRACE=1             one line per tree build / walk / direct-step decision on stderr
 *   NBODY_BUILD_THREADS=k     threads of the host-side tree builder (default: the host's cores, at most 16)
 *   NBODY_TREE_BUILD_HOST=1   build every tree with the host builder instead of the device kernels
 *   NBODY_DIRECT_GRAPH=0      direct steps of small problems as plain launches instead of a replayed hipGraph
 *   NBODY_DIRECT_NEARFAR=0|1|2  near/far split of the direct step's sources: never | by size (default) | always
 *   NBODY_STEP_AHEAD=0        f32 BVH steps phase by phase instead of enqueued whole ahead of the host
 *   NBODY_WALK_SPLIT=0|1|3    big-leaf BVH walk: the fused walk only | one pass through LDS when it pays (default) | whenever possible
 *   NBODY_MULTI_EXCHANGE=peer nbody_create_multi: peer copies instead of RCCL (what nbody_create_multi_ex takes as `exchange`)
 *   NBODY_MULTI_CHUNKS=c      nbody_create_multi: chunks per direct step (default by size; nbody_create_multi_ex's `chunks`)
 * The A/B variants and test hooks the measurements under profiles/ switch between (NBODY_DIRECT_ASM, NBODY_WALK_TILE_*, ...)
 * exist only in the laboratory build, libnbody_hip_lab.so (csrc/env.h, `make lab`); this library ignores them.
 */
#ifndef NBODY_HIP_H
#define NBODY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: nbody_create_multi*, nbody_multi_info, nbody_direct_prep/run_dev, nbody_update_tree_async_f32, nbody_wait,
 *    nbody_get_stream, nbody_delta_decoder_set_max_bodies, nbody_selftest_*_f64 (round 2), nbody_multi_comm_count (round 3);
 * 3: nbody_update_direct_f64, nbody_accel_direct_f64 (the direct O(N^2) step on an f64 context);
 *    nbody_accel_direct_at_f32 / _f64 (the direct sum at arbitrary points) were added under 3: new symbols only, nothing
 *    that existed changed; nbody_tracers_upload_f32 / _f64, nbody_tracers_download_f32 / _f64 and nbody_num_tracers (massless
 *    tracers that step with the bodies) likewise: new symbols only; nbody_render_rgba_tracers, nbody_snapshot_num_tracers,
 *    nbody_snapshot_tracers_f32 / _f64 and nbody_tracers_delta_begin / _pending / _end / _reset (the tracers in the frame, the
 *    snapshot and a delta stream of their own) likewise: new symbols only; nbody_ensemble_* (many small worlds stepped
 *    together, on a handle of their own) likewise: new symbols only; nbody_ensemble64_* (the same in double precision, a
 *    second handle) likewise: new symbols only;
 *    a binding compares nbody_abi_version() with the value it was written against before it binds anything else. */
#define NBODY_ABI_VERSION 3

typedef struct nbody_ctx nbody_ctx;
typedef struct nbody_timer nbody_timer;
typedef struct nbody_host_tree nbody_host_tree;

typedef enum nbody_status {
  NBODY_OK = 0,
  NBODY_ERR_INVALID = -1,    /* bad argument / call order */
  NBODY_ERR_NO_DEVICE = -2,  /* no usable gfx950 device */
  NBODY_ERR_HIP = -3,        /* a HIP runtime call failed (message has the hipError string) */
  NBODY_ERR_DEGENERATE = -4, /* tree build hit the depth cap: > leaf_size coincident points (the
                                reference recurses without bound there, bvh_tree.rs:78-88, quad_tree.rs:159-161) */
  NBODY_ERR_NOMEM = -5
} nbody_status;

/* Arithmetic of the pair function.  Direct sum: all three values below.  Tree walks: AUTO and EXACT use the reference's
 * operations (bit-identical results); FAST is an opt-in that keeps the reference's node tests and interaction lists but
 * evaluates each pair with one reciprocal (tolerance of DESIGN.md §5 instead of bit parity). */
typedef enum nbody_arith {
  NBODY_ARITH_AUTO = 0,  /* FAST, switching per step on device to EXACT when a position is non-finite,
                            >= 2^60 in magnitude, or non-zero below 2^-22 (the inputs on which FAST and the
                            reference's is_normal() skip, main.rs:241-243, could disagree) */
  NBODY_ARITH_FAST = 1,  /* one v_rcp_f32 per pair, fused multiply-adds, sources split over waves;
                            matches the reference to the tolerance in DESIGN.md */
  NBODY_ARITH_EXACT = 2  /* every operation as main.rs:236-252 writes it (IEEE divide, no contraction,
                            is_normal skip), one sequential ascending-j chain per target: bit-identical
                            to the CPU restatement */
} nbody_arith;

/* Which particle order the accelerations of a BVH step are applied in. */
typedef enum nbody_order {
  NBODY_ORDER_AS_WRITTEN = 0, /* reference behaviour: acceleration i is computed for the pre-build
                                 snapshot's particle i and added to the post-build (permuted) particle i
                                 (main.rs:398, :406-416, :419-423) */
  NBODY_ORDER_CONSISTENT = 1  /* acceleration applied to the particle it was computed for */
} nbody_order;

typedef enum nbody_tree_kind {
  NBODY_TREE_BVH = 0,  /* src/bvh_tree.rs (live in the reference) */
  NBODY_TREE_QUAD = 1  /* src/quad_tree.rs build + upward pass (dead code upstream); walk by analogy */
} nbody_tree_kind;

/* Mirrors `struct Counting` (main.rs:74-79): cumulative seconds per phase. */
typedef struct nbody_counting {
  double build_bvh;
  double sum_gravity;
  double post_calculations;
} nbody_counting;

/* Runtime form of the reference's compile-time constants. */
typedef struct nbody_params {
  float theta;       /* THETA = 50.0            main.rs:35   (node accepted when s^2 < d^2*theta*theta) */
  float clamp;       /* 0.001                   main.rs:247-248 */
  int32_t leaf_size; /* TARGET_POINTS = 64      bvh_tree.rs:37 (BVH only; quad leaves hold 8, quad_tree.rs:54) */
  int32_t order;     /* nbody_order, default NBODY_ORDER_AS_WRITTEN */
  int32_t arith;     /* nbody_arith, default NBODY_ARITH_AUTO */
  float quad_root_x; /* root cell of the quad tree: offset (0,0), side HEIGHT = 100000 (main.rs:31) */
  float quad_root_y;
  float quad_root_h;
} nbody_params;

/* ---- lifetime ------------------------------------------------------------------------------------- */
int nbody_abi_version(void);
int nbody_create(nbody_ctx** out, int device_id);
/* Several GPUs behind one handle: device_ids[n_devices] (NULL: 0 .. n_devices-1).  Every call of this
 * header works on the handle as on a single-GPU one — same arguments, same results (bit-identical for tree steps and
 * EXACT arithmetic; FAST direct sums differ by summation order only) — except the *_shard / export / import calls,
 * which belong to hosts that shard by themselves.  The caller still drives it from one thread; the library runs one
 * worker thread per device.
 *   direct steps: device d owns target blocks {c*G + d}; each chunk of G blocks is all-gathered in place (ncclAllGather)
 *     on a communication stream while the next chunk computes;
 *   tree steps: every device builds the same tree, walks and integrates one slice of the tree-ordered targets, one
 *     packed all-gather of {row, position, velocity} per step.
 * nbody_create_multi takes RCCL (NBODY_MULTI_EXCHANGE=peer in the environment selects the peer copies).
 * nbody_create_multi_ex: exchange = NBODY_EXCHANGE_RCCL, or NBODY_EXCHANGE_PEER (hipMemcpyPeerAsync of every block to
 * every peer; also accepts one physical device listed several times — a rehearsal of the sharding on one GPU);
 * chunks = 0 picks the number of chunks per step by size (1 .. 8), 1 .. 16 forces it. */
typedef enum nbody_exchange { NBODY_EXCHANGE_RCCL = 0, NBODY_EXCHANGE_PEER = 1 } nbody_exchange;
int nbody_create_multi(nbody_ctx** out, int n_devices, const int* device_ids);
int nbody_create_multi_ex(nbody_ctx** out, int n_devices, const int* device_ids, int exchange, int chunks);
/* Layout of a context: devices, exchange (-1 for a single-GPU context), chunks per direct step and bodies per target
 * block of the current upload.  Any pointer may be NULL. */
int nbody_multi_info(const nbody_ctx* ctx, int* n_devices, int* exchange, int* chunks, int64_t* block);
/* Ranks of the context's RCCL communicator as RCCL itself reports them (ncclCommCount); 0 for a single-GPU context or the
 * peer-copy exchange. */
int nbody_multi_comm_count(const nbody_ctx* ctx, int* n_ranks);
void nbody_destroy(nbody_ctx* ctx);
const char* nbody_last_error(const nbody_ctx* ctx);
int nbody_default_params(nbody_params* out);
int nbody_set_params(nbody_ctx* ctx, const nbody_params* p);
int nbody_get_params(const nbody_ctx* ctx, nbody_params* out);

/* ---- particle state: replaces `World.particles: Vec<Particle>` (main.rs:37-39) -------------------- */
int nbody_upload_f32(nbody_ctx* ctx, int64_t n, const float* pos_xy, const float* vel_xy, const uint32_t* weight);
int nbody_upload_f64(nbody_ctx* ctx, int64_t n, const double* pos_xy, const double* vel_xy, const uint32_t* weight);
/* Any output pointer may be NULL.  `ids` receives, for each row, the index the particle was uploaded at
 * (a BVH step permutes rows exactly as BVHTree::from permutes `self.particles`, bvh_tree.rs:73-77). */
int nbody_download_f32(nbody_ctx* ctx, float* pos_xy, float* vel_xy, uint32_t* weight, uint32_t* ids);
int nbody_download_f64(nbody_ctx* ctx, double* pos_xy, double* vel_xy, uint32_t* weight, uint32_t* ids);
int64_t nbody_num_particles(const nbody_ctx* ctx);

/* ---- World::update replacements (force + integrate, n_steps times) -------------------------------- */
/* Direct O(N^2): a_i = sum_j calculate_gravity(p_i, p_j, w_j) for j ascending, then main.rs:419-423.
 * (No reference function: this is what bvh_sum_gravity degenerates to at theta = 0) */
int nbody_update_direct_f32(nbody_ctx* ctx, float delta, int n_steps, nbody_counting* counter);
/* The same step on an f64 context (nbody_upload_f64), with T = double throughout; mass is `weight as f64`, the clamp is
 * params.clamp widened to double.  AUTO and EXACT: one ascending-j chain of IEEE additions in double per target, every pair
 * as main.rs:236-252 writes it (two correctly rounded divisions, no contraction, the is_normal skip), integration as
 * main.rs:419-423 without contraction: bit-identical to the CPU restatement.  FAST (opt-in): one v_rcp_f64 + one Newton
 * step per pair, fused multiply-adds, a 2^-700-biased denominator, sources split over waves; |a - a_ref|_1 <= 1e-12 *
 * sum_j |term_ij|_1 per body.  A step whose positions are not all finite, below 2^100 in magnitude and zero or at least
 * 2^-300, or whose clamp is not > 0, runs EXACT instead (decided on the device, per step).  n_steps = 0 or no bodies: a no-op.
 * Not provided for f64: multi-device contexts (NBODY_ERR_INVALID: multi-device direct steps are f32 only), the sharded
 * *_dev entry points, mass classes, the near/far split, and hipGraph replay of small steps.  nbody_update_direct_f32 on
 * an f64 context still fails. */
int nbody_update_direct_f64(nbody_ctx* ctx, double delta, int n_steps, nbody_counting* counter);
/* Barnes-Hut: the linearised tree is the reference's tree, node for node (built on the device; by the host builder
 * for what the device builders decline — NaN positions, trees deeper than they follow — see nbody_last_build_on_device), and the device walks it. */
int nbody_update_tree_f32(nbody_ctx* ctx, int tree_kind, float delta, int n_steps, nbody_counting* counter);
int nbody_update_tree_f64(nbody_ctx* ctx, int tree_kind, double delta, int n_steps, nbody_counting* counter);
/* The reference's loop makes one `update` per iteration and then hands a snapshot to its renderer (main.rs:118-139); a
 * synchronous call per step leaves the GPU idle from the end of one call to the first launch of the next.  The asynchronous
 * form returns as soon as the steps are enqueued — for the f32 BVH: as soon as the host has made its one decision per
 * step, while the walk still runs — so consecutive calls (and nbody_snapshot_begin / nbody_delta_begin between them) run
 * back to back on the device.  The rows are complete for every later call that reads them (each orders itself after
 * the steps); the phase seconds of nbody_get_counting are complete after nbody_wait, which also reports a failure of
 * the device.  On a context made by nbody_create_multi the call is simply synchronous. */
int nbody_update_tree_async_f32(nbody_ctx* ctx, int tree_kind, float delta, int n_steps);
int nbody_wait(nbody_ctx* ctx);

/* ---- sharded Barnes-Hut steps (one process per GPU) ------------------------------------------------
 * Every rank uploads ALL particles and builds the same tree; a rank walks and integrates only its slice
 * [begin, begin+count) of the tree-ordered targets (for the BVH that is rows begin.. of the permuted array, for the
 * quad tree the rows order[begin..]).  After the step the ranks exchange what they changed — nbody_export_slice_dev
 * writes {row index, position, velocity} of the slice into caller-owned DEVICE buffers (count u32 / count xy pairs of
 * the context's precision), the host all-gathers them (RCCL), nbody_import_rows_dev scatters them back — so that all
 * contexts hold the same state again.  nbody-simulation_amd/sharding.py (ShardedTreeStepper) does exactly this. */
int nbody_update_tree_shard_f32(nbody_ctx* ctx, int tree_kind, float delta, int64_t begin, int64_t count, nbody_counting* counter);
int nbody_update_tree_shard_f64(nbody_ctx* ctx, int tree_kind, double delta, int64_t begin, int64_t count, nbody_counting* counter);
int nbody_export_slice_dev(nbody_ctx* ctx, int64_t begin, int64_t count, void* rows_u32, void* pos_xy, void* vel_xy);
int nbody_import_rows_dev(nbody_ctx* ctx, int64_t n_rows, const void* rows_u32, const void* pos_xy, const void* vel_xy);

/* ---- parity hooks: force only, state untouched ----------------------------------------------------- */
/* acc_xy[2*n]: accelerations in current row order. */
int nbody_accel_direct_f32(nbody_ctx* ctx, float* acc_xy);
int nbody_accel_direct_f64(nbody_ctx* ctx, double* acc_xy);  /* arithmetic as nbody_update_direct_f64 */
/* Builds the tree over the current positions (rows are permuted for the BVH, as a step would) and walks
 * it for `n_targets` arbitrary target positions (NULL: the particles themselves, post-build order). */
int nbody_accel_tree_f32(nbody_ctx* ctx, int tree_kind, int64_t n_targets, const float* target_xy, float* acc_xy);
int nbody_accel_tree_f64(nbody_ctx* ctx, int tree_kind, int64_t n_targets, const double* target_xy, double* acc_xy);
/* Direct-sum accelerations of the current bodies at n_targets arbitrary points (x0,y0,x1,y1,...); state untouched.
 * The sources are the bodies in their current row order, each pair calculate_gravity (main.rs:234-253) with the params'
 * clamp; a target is a point without mass or self term (one that sits on a body skips that pair by the reference's rule).
 * Arithmetic as the direct step of the context's precision: EXACT is bit-identical to one ascending-row chain per target;
 * f32 FAST is within the step's tolerance, and AUTO is EXACT for every target when the step would be (a body outside FAST's
 * domain, a clamp below 2^-19), else FAST but for a target outside that domain, which gets its EXACT value; f64 is EXACT
 * unless FAST is asked for, FAST then gated like the f64 step, with the same per-target exception.  Whatever the route, a
 * target's bits depend only on its own position (the bodies, params and build fixed): not on the other targets, their
 * number or order, nor on the number of devices of a multi-device context, which splits the targets into one contiguous
 * block per device.  Targets go through in bounded batches.  Zero bodies: every acceleration is +0.
 * NBODY_ERR_INVALID: ctx NULL, n_targets < 0, a NULL array with n_targets > 0, no particles, the other precision.
 * n_targets == 0 does nothing. */
int nbody_accel_direct_at_f32(nbody_ctx* ctx, int64_t n_targets, const float* target_xy, float* acc_xy);
int nbody_accel_direct_at_f64(nbody_ctx* ctx, int64_t n_targets, const double* target_xy, double* acc_xy);

/* ---- tracers: points without mass that step with the bodies, on the device ------------------------------------
 * m tracers (x0,y0,...; velocities likewise) of the context's precision, kept in device arrays of their own; an upload
 * replaces any earlier set and m == 0 removes them.  While a context holds tracers, every nbody_update_direct_f32 / _f64 and
 * nbody_update_tree_f32 / _f64 step also advances them: a tracer's acceleration is the field of the bodies at their pre-step
 * positions — the snapshot the bodies' own force phase reads; for the tree methods the step's tree, walked at the tracer's
 * position — and it integrates as main.rs:419-423 (v += a*dt; x += v*dt, multiply then add, no contraction).  A tracer has no
 * mass and no self term and exerts nothing.  Rows keep their upload order for ever (a BVH's permutations concern bodies only).
 * Arithmetic: direct steps as nbody_accel_direct_at_* documents it (EXACT one ascending-row chain per tracer; f32 FAST within
 * the step's tolerance; AUTO the step's route, a tracer outside FAST's domain taking its EXACT value; f64 EXACT unless FAST is
 * asked for, then gated like the f64 step with the same per-tracer exception); tree steps as nbody_accel_tree_* with targets.
 * A tracer's route in a step is decided once, from its position before the step.
 * All of it is decided on the device, per step: nothing is read back and no host synchronisation is added between the steps of
 * a call.  A tracer's bits depend on its own state and the bodies alone — not on the other tracers, their number or order.
 * The bodies' rows are bit-identical to the same steps without tracers: the same kernels run in the same order (with tracers
 * present, small direct steps are not replayed from a captured graph and BVH steps are not enqueued ahead of the host; both
 * routes give the same bits as the plain ones).  The FAST partial sums go through a bounded workspace in batches, whatever m
 * is.  The timer of nbody_set_timer keeps bracketing the bodies' dominant kernel only; a direct step's tracer time is booked
 * under sum_gravity with the rest of the call (force and integration are fused), a tree step's tracer walk under sum_gravity
 * and their integration under post_calculations.
 * nbody_upload_* of bodies removes the tracers (a new world).  Tracers leave the device the way bodies do, through calls of their
 * own beside the bodies': nbody_snapshot_begin takes them along (nbody_snapshot_tracers_*), nbody_tracers_delta_* streams their
 * positions as a second NBD1 sequence, nbody_render_rgba_tracers paints them into the frame.  nbody_render_rgba, nbody_delta_* and
 * the parity hooks (nbody_accel_*, nbody_walk_tree_*) still see bodies only and give the same bytes whether tracers exist or not.
 * NBODY_ERR_INVALID (the message names "tracers"): ctx NULL, m < 0, a NULL array with m > 0, the other precision, no particles
 * uploaded, a context made by nbody_create_multi*; and nbody_update_tree_async_f32, nbody_update_tree_shard_*,
 * nbody_export_slice_dev, nbody_import_rows_dev while tracers are present.
 * Download: either pointer may be NULL; upload order, always.  nbody_num_tracers: 0 for NULL or none. */
int nbody_tracers_upload_f32(nbody_ctx* ctx, int64_t m, const float* pos_xy, const float* vel_xy);
int nbody_tracers_upload_f64(nbody_ctx* ctx, int64_t m, const double* pos_xy, const double* vel_xy);
int nbody_tracers_download_f32(nbody_ctx* ctx, float* pos_xy, float* vel_xy);
int nbody_tracers_download_f64(nbody_ctx* ctx, double* pos_xy, double* vel_xy);
int64_t nbody_num_tracers(const nbody_ctx* ctx);

/* ---- ensembles: many small worlds of one size, stepped together in one launch per step (nbody_ensemble_* in f32,
 * nbody_ensemble64_* in f64) -------- A handle of their own each and a header of their own, part of this ABI: declared and
 * documented in nbody_ensemble.h. */
#include "nbody_ensemble.h"

/* Linearised tree of the last build (pre-order; node i's first child is i+1; `skip` is the pre-order index
 * following the subtree).  Any pointer may be NULL; call with all NULL to get the node count. */
typedef struct nbody_tree_view {
  int64_t n_nodes;
  int32_t kind;       /* nbody_tree_kind */
  int32_t max_depth;
} nbody_tree_view;
int nbody_tree_info(const nbody_ctx* ctx, nbody_tree_view* out);
/* geom: BVH [n_nodes][6] = off_x off_y size_x size_y cog_x cog_y; quad [n_nodes][5] = off_x off_y height cog_x cog_y.
 * leaf_first/leaf_count: slice of the tree-ordered particle list; order[n]: upload index of each tree-ordered particle. */
int nbody_tree_export_f32(const nbody_ctx* ctx, float* geom, uint32_t* mass, int32_t* is_leaf, int64_t* leaf_first,
                          int64_t* leaf_count, int64_t* skip, uint32_t* order);
int nbody_tree_export_f64(const nbody_ctx* ctx, double* geom, uint32_t* mass, int32_t* is_leaf, int64_t* leaf_first,
                          int64_t* leaf_count, int64_t* skip, uint32_t* order);

/* Host-side tree build on caller arrays, without a device: the same builder the update calls run (the reference
 * also builds on the host, bvh_tree.rs:56-96).  Returns NBODY_ERR_DEGENERATE (with *out still valid, for
 * inspection) when the depth cap was hit.  `p` may be NULL for the defaults. */
int nbody_host_tree_build_f32(int tree_kind, int64_t n, const float* pos_xy, const uint32_t* weight,
                              const nbody_params* p, nbody_host_tree** out);
int nbody_host_tree_build_f64(int tree_kind, int64_t n, const double* pos_xy, const uint32_t* weight,
                              const nbody_params* p, nbody_host_tree** out);
void nbody_host_tree_free(nbody_host_tree* t);
int nbody_host_tree_info(const nbody_host_tree* t, nbody_tree_view* out);
int nbody_host_tree_export_f32(const nbody_host_tree* t, float* geom, uint32_t* mass, int32_t* is_leaf,
                               int64_t* leaf_first, int64_t* leaf_count, int64_t* skip, uint32_t* order);
int nbody_host_tree_export_f64(const nbody_host_tree* t, double* geom, uint32_t* mass, int32_t* is_leaf,
                               int64_t* leaf_first, int64_t* leaf_count, int64_t* skip, uint32_t* order);

/* The force map alone (main.rs:406-416) over a CALLER'S tree: for a host that keeps its own builder (BVHTree::from +
 * calculate_gravity, bvh_tree.rs:56-158) and hands over only the walk -- SURVEY 8b's nbody_walk_tree.  The tree comes in the
 * layout nbody_tree_export_* writes (pre-order; node i's first child is i + 1; skip[i] the pre-order index after i's subtree;
 * geom BVH [n_nodes][6] = off_x off_y size_x size_y cog_x cog_y, quad [n_nodes][5] = off_x off_y height cog_x cog_y;
 * leaf_first / leaf_count for EVERY node: an inner node's range is its children's ranges one after the other), over the
 * particles uploaded to the context: order[n] = the current row of each tree-ordered particle (the permutation the host's
 * in-place partition made).  The rows are brought into tree order as a build would leave them (BVH) and the tree becomes
 * the context's current tree (nbody_tree_export_* returns it).  target_xy NULL: the particles themselves, acc_xy[2*n] in the
 * context's row order after the call (BVH: tree order, the rows having been permuted; quad: the rows stay where they were).
 * The shape is validated before anything reaches the device (nbody_tree_validate: forward skip links, nested subtrees,
 * two children per BVH root / one to four per quad root, ranges inside the particles, `order` a permutation):
 * NBODY_ERR_INVALID with the reason in nbody_last_error.  Geometry and masses are taken as they are. */
int nbody_walk_tree_f32(nbody_ctx* ctx, int tree_kind, int64_t n_nodes, const float* geom, const uint32_t* mass,
                        const int32_t* is_leaf, const int64_t* leaf_first, const int64_t* leaf_count, const int64_t* skip,
                        const uint32_t* order, int64_t n_targets, const float* target_xy, float* acc_xy);
int nbody_walk_tree_f64(nbody_ctx* ctx, int tree_kind, int64_t n_nodes, const double* geom, const uint32_t* mass,
                        const int32_t* is_leaf, const int64_t* leaf_first, const int64_t* leaf_count, const int64_t* skip,
                        const uint32_t* order, int64_t n_targets, const double* target_xy, double* acc_xy);
/* The shape check of nbody_walk_tree_* on its own (host only, no device): NBODY_OK or NBODY_ERR_INVALID with the first
 * violation written to reason[reason_cap] (may be NULL). */
int nbody_tree_validate(int tree_kind, int64_t n_nodes, const int32_t* is_leaf, const int64_t* leaf_first,
                        const int64_t* leaf_count, const int64_t* skip, int64_t n_particles, const uint32_t* order,
                        char* reason, size_t reason_cap);

/* Walk statistics of the most recent tree walk made while collection was enabled (node visits, accepted nodes,
 * leaf pairs, summed over targets).  `enable` != 0 turns collection on for later walks (it costs three atomics
 * per target), 0 turns it off.  Used to price the walk's algorithmic bytes. */
int nbody_tree_walk_stats(nbody_ctx* ctx, int enable, uint64_t* node_visits, uint64_t* accepted, uint64_t* leaf_pairs);
/* Cumulative phase seconds of this context (the reference prints these once a second, main.rs:149-156). */
int nbody_get_counting(const nbody_ctx* ctx, nbody_counting* out);

/* ---- device-pointer level (caller owns device memory and the stream; used for multi-GPU sharding) -- */
/* One direct step for targets [target_begin, target_begin + n_targets) against all n_sources bodies.
 *   pos_all   float2[n_sources]   all positions (gathered), read only
 *   mass_all  float [n_sources]   weights converted to f32 (u32 -> f32 as `weight as f32`, main.rs:360)
 *   uniform_mass                  > 0 asserts that every entry of mass_all equals this value (the FAST kernel
 *                                 then hoists the multiply out of the sum); < 0 asserts that every entry equals
 *                                 -uniform_mass except a sparse set (at most n/256 bodies: the reference's scene has two
 *                                 heavy bodies among 151 000 of weight 1, main.rs:282-291) — those are found on the
 *                                 device each step and added with their own masses after the equal-mass main pass;
 *                                 0 when masses differ freely or are unknown.  (A context — nbody_upload_* + nbody_update_direct_f32,
 *                                 single- or multi-GPU — goes further by itself: masses that take at most 32 distinct values
 *                                 are handled as mass classes at the equal-mass rate; this device-pointer call has no
 *                                 place to keep the class order and runs the per-body-mass kernel for them.)
 *   vel       float2[n_targets]   this shard's velocities, updated in place
 *   pos_out   float2[n_targets]   this shard's new positions (must not alias pos_all)
 *   acc_out   float2[n_targets]   or NULL
 *   workspace: nbody_direct_workspace_bytes(n_sources, n_targets) bytes, 256-B aligned, reusable across calls
 * delta == 0 with vel == pos_out == NULL computes accelerations only.
 * `stream` is a hipStream_t.  `arith` is an nbody_arith; AUTO/EXACT semantics as above. */
size_t nbody_direct_workspace_bytes(int64_t n_sources, int64_t n_targets);
int nbody_direct_step_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all,
                          float uniform_mass, int64_t target_begin, int64_t n_targets, void* vel, void* pos_out, void* acc_out,
                          float delta, float clamp, int arith, void* workspace, size_t workspace_bytes,
                          nbody_timer* timer /* may be NULL */);
/* The same step in two parts, for hosts that cut a rank's targets into several blocks (to start the exchange of one
 * block while the next computes): ONE preparation over all positions (hazard scan, near/far split, decision word),
 * then one run per block.  n_targets_total = all targets this rank computes in the step (decides whether the near/far
 * split pays), n_targets_max = the largest block (sizes the workspace: nbody_direct_workspace_bytes(n_sources,
 * n_targets_max)); both calls must be given the same two values.  nbody_direct_step_dev = prep + one run. */
int nbody_direct_prep_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all, float uniform_mass,
                          int64_t n_targets_total, int64_t n_targets_max, float clamp, int arith, void* workspace,
                          size_t workspace_bytes);
int nbody_direct_run_dev(void* stream, int64_t n_sources, const void* pos_all, const void* mass_all, float uniform_mass,
                         int64_t target_begin, int64_t n_targets, void* vel, void* pos_out, void* acc_out, float delta,
                         float clamp, int arith, int64_t n_targets_total, int64_t n_targets_max, void* workspace,
                         size_t workspace_bytes, nbody_timer* timer /* may be NULL */);
/* The hipStream_t a context enqueues its steps on (a multi context: its first device's).  A host that mixes the
 * context's calls with its own stream-ordered work (a collective on the exported slice, say) runs that work on this
 * stream, or orders against it with events, instead of synchronising the device. */
void* nbody_get_stream(const nbody_ctx* ctx);
/* Decision words of the last nbody_direct_step_dev call on that workspace (waits for the stream):
 * out = {hazard flag, split fallback flag, number of near sources, state} with state 0 = near/far split (the main
 * pass skips the clamp for sources proven far from every other body, the near ones are added with it), 1 = one
 * clamped FAST pass, 2 = EXACT kernel.  Parity/diagnostic hook. */
int nbody_direct_workspace_peek(void* stream, const void* workspace, int32_t out[4]);
/* u32 weights -> f32 masses on device (the `as f32` of main.rs:360). */
int nbody_weights_to_mass_dev(void* stream, int64_t n, const void* weight_u32, void* mass_f32);

/* ---- snapshot hand-off (main.rs:136-139) ---------------------------------------------------------------- */
/* The reference's sim thread clones `world.particles` for the render thread whenever the bounded channel has room
 * (`if !tx.is_full() { tx.try_send((world.particles.clone(), updates, counter.clone())) }`) and keeps stepping.
 * nbody_snapshot_begin copies the current rows aside on the device (ordered after the last step) and starts their
 * transfer to pinned host memory on a second stream; steps issued afterwards run alongside that transfer.
 * nbody_snapshot_end waits for it and hands the rows out (any pointer may be NULL) together with the number of steps
 * the context had done when the snapshot was taken (`updates`).  One snapshot in flight per context: begin while one
 * is pending fails with NBODY_ERR_INVALID — "channel full", skip it as the reference does (nbody_snapshot_pending). */
int nbody_snapshot_begin(nbody_ctx* ctx);
int nbody_snapshot_pending(const nbody_ctx* ctx);
int nbody_snapshot_end_f32(nbody_ctx* ctx, float* pos_xy, float* vel_xy, uint32_t* weight, uint32_t* ids, uint64_t* step_out);
int nbody_snapshot_end_f64(nbody_ctx* ctx, double* pos_xy, double* vel_xy, uint32_t* weight, uint32_t* ids, uint64_t* step_out);

/* The tracers of the pending snapshot.  nbody_snapshot_begin on a context that holds tracers copies their positions and
 * velocities aside too — on the device, in the same place in stream order as the rows — and sends them to pinned host memory
 * on the copy stream with the rest.  These calls are valid while a snapshot is pending: they wait for the transfer and copy
 * out the tracers as they were at begin, in upload order (either pointer may be NULL), whatever happened to the context's
 * tracers since (a tracer upload or removal, a body upload).  They do not end the snapshot: nbody_snapshot_end_* still does.
 * nbody_snapshot_num_tracers: tracers of the pending snapshot, 0 if none is pending; with 0 tracers the copy-out succeeds and
 * writes nothing.  NBODY_ERR_INVALID: ctx NULL, a context made by nbody_create_multi*, no snapshot pending, the other precision. */
int64_t nbody_snapshot_num_tracers(const nbody_ctx* ctx);
int nbody_snapshot_tracers_f32(nbody_ctx* ctx, float* pos_xy, float* vel_xy);
int nbody_snapshot_tracers_f64(nbody_ctx* ctx, double* pos_xy, double* vel_xy);

/* ---- delta snapshots (the commented experiment of main.rs:107-134) ------------------------------------------ */
/* Upstream tried, and left commented out, taking the difference of the positions across an update and printing its
 * zstd-compressed size.  There is no behaviour or format to match; this is the device-side counterpart of that idea
 * for the snapshot hand-off above: the POSITIONS of a snapshot, in upload (id) order, as a lossless stream of bit
 * planes of the change against the previous delta snapshot (format "NBD1": csrc/delta_codec.h, restated in
 * oracle/delta_codec.py).  The first stream after an upload or nbody_delta_reset is a key frame (the change against
 * all-zero state); every later one needs all streams since the key frame applied in order.
 * nbody_delta_begin encodes on the device (ordered after the last step; waits for the encoder to learn the size) and
 * starts the transfer of the stream to pinned host memory on the copy stream; nbody_delta_end waits for it and copies
 * the stream out.  *bytes_out receives the stream's size; if cap is smaller the call fails with NBODY_ERR_INVALID
 * and the stream stays pending (nbody_delta_bound gives the worst case for n bodies).  One in flight per context. */
int nbody_delta_begin(nbody_ctx* ctx);
int nbody_delta_pending(const nbody_ctx* ctx);
int nbody_delta_end(nbody_ctx* ctx, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* step_out);
int nbody_delta_reset(nbody_ctx* ctx);
size_t nbody_delta_bound(int64_t n, int is_f64);
/* The same for the tracers' positions: a second sequence of NBD1 streams with key arrays and a key-frame sequence of its own.
 * The header's body count is m and the positions are the tracers' in upload order; semantics as nbody_delta_* — ordered after
 * the last step, one tracers stream in flight per context (beside the bodies' one: one of each may be pending at once, taken
 * in either order), a too small cap leaves the stream pending (nbody_delta_bound(m, is_f64) sizes it), the first stream after
 * nbody_tracers_upload_* or nbody_tracers_delta_reset is a key frame.  The bodies' streams are the same bytes whether or not
 * tracers exist or a tracers stream is in flight.  The receiving side is a second nbody_delta_decoder.
 * NBODY_ERR_INVALID: ctx NULL, a context made by nbody_create_multi*, begin without tracers or while a tracers stream is
 * pending, end with none pending, reset while one is pending. */
int nbody_tracers_delta_begin(nbody_ctx* ctx);
int nbody_tracers_delta_pending(const nbody_ctx* ctx);
int nbody_tracers_delta_end(nbody_ctx* ctx, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* step_out);
int nbody_tracers_delta_reset(nbody_ctx* ctx);
/* The receiving side (host only, no device needed): a decoder holds the keys of the last two snapshots. */
typedef struct nbody_delta_decoder nbody_delta_decoder;
nbody_delta_decoder* nbody_delta_decoder_create(void);
void nbody_delta_decoder_destroy(nbody_delta_decoder* dec);
/* Applies one stream.  A malformed, truncated or out-of-sequence stream (a delta before any key frame, another n or
 * element size than the state) fails with NBODY_ERR_INVALID and leaves the decoder as it was. */
int nbody_delta_decoder_apply(nbody_delta_decoder* dec, const uint8_t* stream, size_t bytes);
/* The stream is untrusted input: a header may claim up to 2^31 - 1 bodies with an all-zero-width payload of a few MB,
 * i.e. ~100 GB of decoder state.  A stream claiming more than max_bodies is refused before anything is allocated
 * (default 2^31 - 1; a failed allocation is also a refusal, with the state untouched). */
int nbody_delta_decoder_set_max_bodies(nbody_delta_decoder* dec, int64_t max_bodies);
const char* nbody_delta_decoder_error(const nbody_delta_decoder* dec);
int64_t nbody_delta_decoder_count(const nbody_delta_decoder* dec);   /* bodies of the current state, -1 before a key frame */
int nbody_delta_decoder_is_f64(const nbody_delta_decoder* dec);
uint64_t nbody_delta_decoder_step(const nbody_delta_decoder* dec);
/* Positions of the current state, x y per body in id order; the precision must be the stream's. */
int nbody_delta_decoder_positions_f32(const nbody_delta_decoder* dec, float* pos_xy);
int nbody_delta_decoder_positions_f64(const nbody_delta_decoder* dec, double* pos_xy);

/* ---- frame raster: the reference's draw() (main.rs:41-72) ---------------------------------------------- */
/* A render_px x render_px RGBA8 frame of the current rows, exactly as draw() paints `world.particles` (row order
 * = the order nbody_download returns): rows inside [0, height)^2 land on pixel (y as u32 / cell) * render_px +
 * (x as u32 / cell), cell = height / render_px (HEIGHT = 100000, RENDER_HEIGHT = 1250 upstream, main.rs:31-32);
 * weight > 10 paints (0,255,0,255); lighter rows paint R = 255, G = B = 255 - (0x10 + min(((|vx|+|vy|)*10) as u8,
 * 0xef)) of the LAST such row on the pixel, alpha = min(10 * rows, 250).  rgba_out: host, render_px^2 * 4 bytes.
 * render_px must divide height (upstream indexes out of range otherwise). */
int nbody_render_rgba(nbody_ctx* ctx, uint32_t height, uint32_t render_px, uint8_t* rgba_out);
/* The frame with the tracers in it: draw() of the rows followed by the context's tracers, in upload order, as rows n .. n+m-1
 * of weight 1.  A tracer is a light row: it adds 10 to its pixel's alpha (saturating at 250 with the light bodies there),
 * colours the pixel if it is the last light row on it, and never turns a heavy body's green pixel.  Without tracers the frame
 * is nbody_render_rgba's.  Arguments as nbody_render_rgba; the row packing holds 2^24 rows, so n + m > 2^24 is refused before
 * anything is launched (the message names "tracers"), as nbody_render_rgba refuses n > 2^24.  NBODY_ERR_INVALID also: ctx
 * NULL, a context made by nbody_create_multi*. */
int nbody_render_rgba_tracers(nbody_ctx* ctx, uint32_t height, uint32_t render_px, uint8_t* rgba_out);
/* Same on caller-owned device arrays and stream (n <= 2^24 rows; work_u32: 2 * render_px^2 u32 scratch;
 * rgba_dev: render_px^2 * 4 bytes).  Asynchronous. */
int nbody_render_rgba_dev(void* stream, int64_t n, int is_f64, const void* pos_xy, const void* vel_xy, const void* weight_u32,
                          uint32_t height, uint32_t render_px, void* work_u32, void* rgba_dev);

/* ---- self-test hooks (host only unless they say otherwise) --------------------------------------------------- */
/* The device BVH build reproduces the sequential f32 sum of bvh_tree.rs:58-61 with a parallel scan
 * (csrc/exact_sum.h).  This runs the same scan functions on the CPU, `tile` addends per scan and `seq_run` plain
 * adds after every restart, so the CPU tests can check them against the plain loop. */
int nbody_selftest_exact_sum(const float* x, int64_t n, int tile, int seq_run, float* out_sum, int64_t* out_restarts);
/* The chunked variant long chains use (runs prepared per chunk for a PREDICTED binade — two runs and a few real adds in
 * between where the prefix crosses a power of two — used only when the prediction and the run's bounds hold for the true
 * state): same functions on the CPU; *out_runs_used counts the runs that were applied. */
int nbody_selftest_exact_sum_chunked(const float* x, int64_t n, int chunk, float* out_sum, int64_t* out_runs_used);
/* The f64 twin (csrc/exact_sum64.h: 53-bit significands, 64-bit increments), which the device build of f64 BVHs runs. */
int nbody_selftest_exact_sum_f64(const double* x, int64_t n, int tile, int seq_run, double* out_sum, int64_t* out_restarts);
/* ... and its segmented form for long chains (runs prepared per segment for a predicted binade, used only when the
 * prediction and the run's bounds hold for the true state); *out_runs_used counts the runs that were applied. */
int nbody_selftest_exact_sum_f64_segmented(const double* x, int64_t n, int seg, double* out_sum, int64_t* out_runs_used);
/* The exact kernels divide by csrc/div_pair.h: (nx / den, ny / den), the two IEEE f32 divisions of main.rs:252 with their
 * multiply-adds issued as packed instructions.  This runs it on device `device` over n host triples and hands the quotients
 * back, so that a test can compare them bit for bit with the host's IEEE division (needs a GPU). */
int nbody_selftest_div_pair(int device, const float* nx, const float* ny, const float* den, int64_t n, float* qx, float* qy);
/* The one-pass tree walk cuts its waves by an estimate: hist[ids[t]] >> shift terms for target t (t < n, ids distinct indices
 * below hist_n).  This runs the walk's PREPARATION alone on device `device` — no walk kernel, no tree — by one of its routes:
 * 0 the library scan, the wrap check and the total (a plain step); 1 the library scan and the check whose last work-group also
 * concludes on the build (a step enqueued ahead, more than 2^24 targets); 2 the single-pass scan that does all of it (a step
 * enqueued ahead; n <= 2^24).  Routes 1 and 2 judge a build described by the named values (the function lays them out as the
 * 128-word flags block a step packs: level counters from word 32 on, every unused word a value of its own) and afterwards
 * clear `clear_words` (128 .. 65536) words starting at that block.  hist_n <= 2^22.  keep_scratch != 0: the scratch block of
 * this thread's previous such call is used again if it is large enough (the scan's state area is zeroed once per allocation
 * only) and stays allocated for the next; keep_scratch == 0: a fresh block, freed (with any kept one) before returning.
 * Out: off[n] (the exclusive scan), info[8], verdict[2], pack[2 + 128 + 8] (verdict | flags block | info), flags[128] (the
 * block as built), clear[clear_words] (that region afterwards), used[4] = {extra waves, grid waves, 1 if the scratch was kept,
 * 0}.  Route 0 leaves verdict and pack zero and the clear region as built.  Needs a GPU. */
int nbody_selftest_walk_estimate(int device, const uint32_t* hist, int64_t hist_n, const uint32_t* ids, int64_t n, int shift, int route,
                                 int nodes, int node_count, int fallback, int bad_index, int long_nodes_at_level_end, int level_end,
                                 int node_cap, int keep_scratch, uint32_t* out_off, int32_t* out_info, int32_t* out_verdict,
                                 int32_t* out_pack, int32_t* out_flags, int32_t* out_clear, int64_t clear_words, int64_t* out_used);
/* The near/far split of a direct step's sources alone on device `device` — no main pass, no finish — over n host bodies
 * (1 <= n <= 2^24), called exactly as a step without mass classes calls it.  pos_xy: x y per body; mass: n floats or NULL
 * (needed when heavy_base > 0 or with_minv); heavy_base > 0: bodies of another mass are near too (the sparse route); use_hazard:
 * FAST's domain check rides along; couples: the far copy in couples {xA, xB, yA, yB}, padded to a multiple of 16 slots;
 * with_minv (couples only): the inverse masses beside it.  The scratch holds 0xA5 bytes before the call, the flag words zeros.
 * Out: flags[4] as nbody_direct_workspace_peek lists them, is_near[n], scan[n] (its exclusive sum), near_list[n] of which the
 * first flags[2] entries are written, far: 2 * 16 * ceil(n / 16) floats with couples, 2 n without, minv: 16 * ceil(n / 16)
 * floats (with_minv; else may be NULL).  Needs a GPU. */
int nbody_selftest_nearfar(int device, const float* pos_xy, const float* mass, int64_t n, float heavy_base, float clamp, int use_hazard,
                           int couples, int with_minv, int32_t* out_flags, uint32_t* out_is_near, uint32_t* out_scan,
                           uint32_t* out_near_list, float* out_far, float* out_minv);
/* Restarts of that scan during the last device BVH build of this context (diagnostic; 0 after a host build). */
int nbody_bvh_build_restarts(const nbody_ctx* ctx);
/* 1 if the last tree build of this context ran on the device, 0 if the host builder did it (the device builders
 * decline what they cannot express, e.g. NaN positions or very deep trees; NBODY_TREE_BUILD_HOST=1 forces the host). */
int nbody_last_build_on_device(const nbody_ctx* ctx);

/* ---- kernel timing (bench.py's roofline leg) -------------------------------------------------------- */
/* A timer brackets every launch of the dominant kernel of a call (direct: direct_fast / direct_exact; tree:
 * the walk kernel) with HIP events recorded on the stream the kernel is launched on. */
int nbody_timer_create(nbody_timer** out);
void nbody_timer_destroy(nbody_timer* t);
/* Waits for the recorded events; average milliseconds per launch and launch count since the last reset. */
int nbody_timer_read(nbody_timer* t, int reset, double* avg_ms, int64_t* launches);
/* Context-level calls time their dominant kernel with `t` (NULL turns timing off). */
int nbody_set_timer(nbody_ctx* ctx, nbody_timer* t);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_H */
