/*
 * nbody_ensemble.h — the ensemble calls of the C ABI of include/nbody_hip.h (which includes this file where its types are
 * complete: include nbody_hip.h, not this).  New symbols under NBODY_ABI_VERSION 3; conventions as nbody_hip.h states them.
 */
#ifndef NBODY_ENSEMBLE_H
#define NBODY_ENSEMBLE_H
#ifndef NBODY_HIP_H
#error "include nbody_hip.h: it includes nbody_ensemble.h after the types these declarations need"
#endif

/* ---- ensembles: many small worlds of one size, stepped together ------------------------------------------------
 * The same scene under many seeds, a sweep over initial conditions, many independent clusters: worlds too small to fill the
 * device one at a time (below a few thousand bodies a direct step is a handful of launches that cannot occupy it, whatever the
 * kernel does).  An ensemble holds n_worlds worlds of n_bodies bodies each in world-major device arrays and steps ALL of them
 * with one launch per step: the grid runs over worlds x target tiles and every block stages its world's sources whole in LDS.
 * The handle is opaque and its own (no nbody_ctx is involved); it belongs to one host thread at a time; calls are synchronous.
 *   Step.  Every world takes the step of nbody_update_direct_f32, independently of the others: a_i = sum_j
 *     calculate_gravity(p_i, p_j, w_j) over the bodies of its own world, j ascending (main.rs:234-253), then main.rs:419-423
 *     (multiply then add, no contraction).  Rows never move, so there are no ids.
 *   Limits.  1 <= n_bodies <= 4096 (a world's positions and masses are 48 KB at the top size and stage whole in LDS; above
 *     that a context per world is the tool — where the crossover lies is unmeasured), n_worlds >= 1, n_worlds * n_bodies <= 2^26.
 *     Anything outside gives NBODY_ERR_INVALID before anything is allocated, and the message names "ensemble".
 *   EXACT.  Every world is bit-identical to the CPU restatement's update_direct of that world alone.
 *   FAST.  Every body within the tolerance of DESIGN.md (2e-5 of sum_j |term_ij|): one v_rcp_f32 per pair, fused multiply-adds,
 *     the 2^-90 biased denominator.
 *   AUTO.  FAST, decided per world, per step, on the device: a world takes EXACT for a step when one of its positions is outside
 *     FAST's domain (non-finite, >= 2^60 in magnitude, or non-zero below 2^-22) at the start of that step; with a clamp below
 *     2^-19, or NaN, every world takes EXACT (FAST asked for by name, too).  Nothing is read back and there is no host
 *     synchronisation between the steps of a call.
 *   Independence.  A world's bits depend only on its own rows, n_bodies and the params: not on the number of worlds, its index
 *     among them, the other worlds' contents or routes, nor on how the steps are split over calls.  This holds for FAST too: its
 *     summation order is a fixed function of n_bodies.
 *   Trivial calls and errors.  n_steps == 0 is a no-op; an update, accel or download before an upload is NBODY_ERR_INVALID.  There
 *     is no CPU fallback: without a gfx950 device nbody_ensemble_create fails with NBODY_ERR_NO_DEVICE.  A NULL handle gives
 *     NBODY_ERR_INVALID (0 from nbody_ensemble_num_worlds / _num_bodies).  nbody_ensemble_last_error(NULL): the last failed
 *     nbody_ensemble_create on this thread.
 *   Booking.  Force and integration are fused, so the whole call's seconds are booked under sum_gravity, as the direct step
 *     books them (`counter` may be NULL).
 *   Params.  nbody_default_params' values at creation; clamp and arith are used, the rest is kept and ignored.
 *   Not offered: f64 on this handle (nbody_ensemble64_* below is the double-precision sibling); worlds of different sizes on
 *     this handle (nbody_ragged_* at the end of this file steps them together); tree methods;
 *     tracers on this handle (nbody_restricted_* at the end of this file); several devices; asynchronous snapshots and delta streams
 *     on a copy stream (the synchronous streams are nbody_deltas_* and the frames nbody_frames_*, both at the end of this
 *     file); hipGraph replay.  The library reads no environment variable for any of this.  (A time step, a clamp and a number
 *     of steps per world: nbody_sweep_* at the end of this file.  A record per world of what a study ends in — moments, extent,
 *     separations: nbody_summary_* at the end of this file.  Every target's nearest neighbour and the pairs the clamp
 *     altered: nbody_encounters_* at the end of this file.)
 * Arrays are world-major, [n_worlds][n_bodies] rows, pos / vel interleaved x,y; weight may be NULL (all 1); an upload replaces
 * the previous ensemble, whatever its shape. */
typedef struct nbody_ensemble nbody_ensemble;
int nbody_ensemble_create(nbody_ensemble** out, int device_id);
void nbody_ensemble_destroy(nbody_ensemble* e);
const char* nbody_ensemble_last_error(const nbody_ensemble* e);
int nbody_ensemble_set_params(nbody_ensemble* e, const nbody_params* p);
int nbody_ensemble_get_params(const nbody_ensemble* e, nbody_params* out);
int nbody_ensemble_upload_f32(nbody_ensemble* e, int64_t n_worlds, int64_t n_bodies, const float* pos_xy, const float* vel_xy,
                              const uint32_t* weight);
int nbody_ensemble_download_f32(nbody_ensemble* e, float* pos_xy, float* vel_xy); /* either may be NULL */
int64_t nbody_ensemble_num_worlds(const nbody_ensemble* e);
int64_t nbody_ensemble_num_bodies(const nbody_ensemble* e);                       /* per world */
int nbody_ensemble_update_f32(nbody_ensemble* e, float delta, int n_steps, nbody_counting* counter);
int nbody_ensemble_accel_f32(nbody_ensemble* e, float* acc_xy);                   /* force only, state untouched */

/* ---- ensembles in f64: the double-precision sibling, a handle of its own ------------------------------------------
 * Everything above holds with these differences (limits, conventions, errors, booking and the "not offered" list are the same;
 * a study of how fast neighbouring trajectories separate wants a state whose own rounding does not decide the answer).
 *   Step.  Every world takes the step of nbody_update_direct_f64: the pair of main.rs:234-253 in T = double (two correctly
 *     rounded divisions, no contraction, the is_normal skip), mass `weight as f64`, the clamp params.clamp widened to double,
 *     then main.rs:419-423, multiply then add.
 *   EXACT and AUTO.  One ascending-j chain of IEEE additions per target: every world is bit-identical to the CPU restatement's
 *     update_direct of that world alone on float64 arrays.  AUTO is EXACT, as it is for an f64 context.
 *   FAST (opt-in).  |a - a_ref|_1 <= 1e-12 * sum_j |term_ij|_1 per body: v_rcp_f64 plus one Newton step, fused
 *     multiply-adds, the 2^-700 biased denominator.  Gated per world, per step, on the device: a world with a position outside
 *     the f64 FAST domain (non-finite, >= 2^100 in magnitude, or non-zero below 2^-300) at the start of a step takes EXACT for
 *     that step; with a clamp that is not > 0, or NaN, every world takes EXACT.  FAST's order of additions is a fixed function
 *     of n_bodies (ensemble64_kernels.hip), so independence holds for it too.
 *   Staging.  A world's positions and u32 weights are 80 KB of LDS at n_bodies = 4096 (two blocks are the CU's 160 KB exactly:
 *     the kernel uses no other LDS).
 *   The two handles are independent: an nbody_ensemble and an nbody_ensemble64 (and contexts) may be used side by side. */
typedef struct nbody_ensemble64 nbody_ensemble64;
int nbody_ensemble64_create(nbody_ensemble64** out, int device_id);
void nbody_ensemble64_destroy(nbody_ensemble64* e);
const char* nbody_ensemble64_last_error(const nbody_ensemble64* e);
int nbody_ensemble64_set_params(nbody_ensemble64* e, const nbody_params* p);
int nbody_ensemble64_get_params(const nbody_ensemble64* e, nbody_params* out);
int nbody_ensemble64_upload(nbody_ensemble64* e, int64_t n_worlds, int64_t n_bodies, const double* pos_xy, const double* vel_xy,
                            const uint32_t* weight);
int nbody_ensemble64_download(nbody_ensemble64* e, double* pos_xy, double* vel_xy); /* either may be NULL */
int64_t nbody_ensemble64_num_worlds(const nbody_ensemble64* e);
int64_t nbody_ensemble64_num_bodies(const nbody_ensemble64* e);                     /* per world */
int nbody_ensemble64_update(nbody_ensemble64* e, double delta, int n_steps, nbody_counting* counter);
int nbody_ensemble64_accel(nbody_ensemble64* e, double* acc_xy);                    /* force only, state untouched */

/* ---- ragged ensembles: worlds of different sizes stepped together, a handle of its own (f32) ----------------------
 * A sweep over N, clusters drawn from a mass function, halos cut out of a larger run: worlds that differ in size.  Padding them
 * to one size is wrong (a padded body of weight 0 still moves EXACT's chain and FAST's order of additions: both are functions
 * of n), and one nbody_ensemble per distinct size is one launch chain per size again.  A ragged ensemble holds n_worlds worlds
 * of n_bodies[k] bodies each and steps all of them with at most NBODY_RAGGED_MAX_LAUNCHES launches per step.
 *   Arrays.  The worlds' rows come one after another in world order, with no padding: world k's rows are [off_k, off_k + n_k)
 *     with off_k the sum of the sizes before it; pos / vel interleaved x,y; weight may be NULL (all 1).  An upload replaces the
 *     previous ragged ensemble, whatever its sizes.
 *   Limits.  1 <= n_bodies[k] <= 4096 for every world, n_worlds >= 1, the sizes add up to at most 2^26 rows.  Anything outside
 *     gives NBODY_ERR_INVALID before anything is allocated, and the message names "ragged".
 *   Contract.  Step, EXACT, FAST, AUTO (per world, per step, on the device), booking, params, trivial calls and errors, no CPU
 *     path (nbody_ragged_create fails with NBODY_ERR_NO_DEVICE without a gfx950 device), NULL handle (NBODY_ERR_INVALID; 0 from
 *     nbody_ragged_num_worlds / _num_rows; nbody_ragged_last_error(NULL): the last failed nbody_ragged_create or
 *     nbody_ragged_plan on this thread): as the ensemble above states them, word for word.
 *   Independence.  A world's bits depend only on its own rows, its own size and the params.  They do not depend on the other
 *     worlds' sizes, contents, routes or order.  They do not depend on which launch the world falls in.  They do not depend on
 *     how steps are split over calls.
 *   EXACT.  Every world is bit-identical to the CPU restatement's update_direct of that world alone.
 *   FAST.  Every world is bit-identical to nbody_ensemble_* holding that world alone (the two kernels share one body; FAST's
 *     order of additions is a fixed function of the world's n_bodies), hence within the ensemble's tolerance.
 *   Launches.  Worlds are grouped by the LDS they need, in size order: n <= 128, <= 256, <= 512, <= 1024, <= 2048, <= 4096; every
 *     class that has a world is one launch per step, under the LDS of its largest member, and within a launch one block is one
 *     (world, tile) work item of a table built at upload.  An upload through this handle always takes the ragged kernel, also
 *     when all sizes are equal.  nbody_ragged_plan shows the plan the handle uses: for every world its launch and the first of
 *     its (contiguous) blocks in that launch, the number of launches, and per launch (arrays of NBODY_RAGGED_MAX_LAUNCHES, zero
 *     past n_launches) the dynamic LDS and the number of blocks.  It is pure host code: no device, no handle, every output
 *     pointer may be NULL; sizes outside the limits give NBODY_ERR_INVALID and nothing is written.
 *   Not offered on this handle: f64 (nbody_ragged64_* below is the double-precision sibling),
 *     tracers (nbody_rr_* at the end of this file steps worlds of different sizes with tracers of their own), tree methods,
 *     several devices, and what the ensemble above does not offer either. */
#define NBODY_RAGGED_MAX_LAUNCHES 6
typedef struct nbody_ragged nbody_ragged;
int nbody_ragged_create(nbody_ragged** out, int device_id);
void nbody_ragged_destroy(nbody_ragged* e);
const char* nbody_ragged_last_error(const nbody_ragged* e);
int nbody_ragged_set_params(nbody_ragged* e, const nbody_params* p);
int nbody_ragged_get_params(const nbody_ragged* e, nbody_params* out);
int nbody_ragged_upload_f32(nbody_ragged* e, int64_t n_worlds, const int64_t* n_bodies /*[n_worlds]*/, const float* pos_xy,
                            const float* vel_xy, const uint32_t* weight);
int nbody_ragged_download_f32(nbody_ragged* e, float* pos_xy, float* vel_xy);     /* either may be NULL */
int64_t nbody_ragged_num_worlds(const nbody_ragged* e);
int64_t nbody_ragged_num_rows(const nbody_ragged* e);                             /* the sum of the sizes */
int nbody_ragged_sizes(const nbody_ragged* e, int64_t* n_bodies_out /*[num_worlds]*/);
int nbody_ragged_update_f32(nbody_ragged* e, float delta, int n_steps, nbody_counting* counter);
int nbody_ragged_accel_f32(nbody_ragged* e, float* acc_xy);                       /* force only, state untouched */
int nbody_ragged_plan(int64_t n_worlds, const int64_t* n_bodies, int32_t* launch_of_world, int64_t* first_block_of_world,
                      int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch);

/* ---- ragged ensembles in f64: double-precision worlds of different sizes, a handle of its own ---------------------
 * The ragged ensemble above in double precision: arrays, limits, launches (the same six classes, at most
 * NBODY_RAGGED_MAX_LAUNCHES per step), independence, booking, params, trivial calls and errors as stated there, with the message
 * naming "ragged"; no CPU path (nbody_ragged64_create fails with NBODY_ERR_NO_DEVICE without a gfx950 device); NULL handle
 * (NBODY_ERR_INVALID; 0 from nbody_ragged64_num_worlds / _num_rows; nbody_ragged64_last_error(NULL): the last failed
 * nbody_ragged64_create or nbody_ragged64_plan on this thread — a slot of its own, apart from nbody_ragged_*'s and
 * nbody_ensemble64_*'s).  The arithmetic is nbody_ensemble64_*'s, word for word:
 *   Step.  Every world takes the step of nbody_update_direct_f64: the pair of main.rs:234-253 in T = double (two correctly
 *     rounded divisions, no contraction, the is_normal skip), mass `weight as f64`, the clamp params.clamp widened to double,
 *     then main.rs:419-423, multiply then add.
 *   EXACT and AUTO.  One ascending-j chain of IEEE additions per target: every world is bit-identical to the CPU restatement's
 *     update_direct of that world alone on float64 arrays.  AUTO is EXACT, as it is for an f64 context.
 *   FAST (opt-in).  |a - a_ref|_1 <= 1e-12 * sum_j |term_ij|_1 per body: v_rcp_f64 plus one Newton step, fused
 *     multiply-adds, the 2^-700 biased denominator.  Gated per world, per step, on the device: a world with a position outside
 *     the f64 FAST domain (non-finite, >= 2^100 in magnitude, or non-zero below 2^-300) at the start of a step takes EXACT for
 *     that step; with a clamp that is not > 0, or NaN, every world takes EXACT.  Every world is bit-identical to
 *     nbody_ensemble64_* holding that world alone (the two kernels share one body; FAST's order of additions is a fixed
 *     function of the world's n_bodies).
 *   Launches.  Per launch the dynamic LDS is that of its largest member at 20 bytes a body, rows padded to a multiple of 8:
 *     at most 2 560, 5 120, 10 240, 20 480, 40 960 and 81 920 B for the six classes (the kernel uses no other LDS).
 *     nbody_ragged64_plan is nbody_ragged_plan under these sizes. */
typedef struct nbody_ragged64 nbody_ragged64;
int nbody_ragged64_create(nbody_ragged64** out, int device_id);
void nbody_ragged64_destroy(nbody_ragged64* e);
const char* nbody_ragged64_last_error(const nbody_ragged64* e);
int nbody_ragged64_set_params(nbody_ragged64* e, const nbody_params* p);
int nbody_ragged64_get_params(const nbody_ragged64* e, nbody_params* out);
int nbody_ragged64_upload(nbody_ragged64* e, int64_t n_worlds, const int64_t* n_bodies /*[n_worlds]*/, const double* pos_xy,
                          const double* vel_xy, const uint32_t* weight);
int nbody_ragged64_download(nbody_ragged64* e, double* pos_xy, double* vel_xy);   /* either may be NULL */
int64_t nbody_ragged64_num_worlds(const nbody_ragged64* e);
int64_t nbody_ragged64_num_rows(const nbody_ragged64* e);                         /* the sum of the sizes */
int nbody_ragged64_sizes(const nbody_ragged64* e, int64_t* n_bodies_out /*[num_worlds]*/);
int nbody_ragged64_update(nbody_ragged64* e, double delta, int n_steps, nbody_counting* counter);
int nbody_ragged64_accel(nbody_ragged64* e, double* acc_xy);                      /* force only, state untouched */
int nbody_ragged64_plan(int64_t n_worlds, const int64_t* n_bodies, int32_t* launch_of_world, int64_t* first_block_of_world,
                        int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch);

/* ---- restricted ensembles: tracers that step with each world, a handle of its own (f32) ---------------------------
 * The restricted problem under many seeds or parameters: a few massive bodies and thousands of test particles per world — ring
 * and belt stability maps, capture cross-sections, scattering sweeps.  A restricted ensemble holds n_worlds worlds of n_bodies
 * bodies each, as nbody_ensemble_* does (1 <= n_bodies <= 4096, n_worlds * n_bodies <= 2^26), and beside them n_tracers massless
 * points per world (n_tracers >= 0, the same for every world, n_worlds * n_tracers <= 2^26).  All arrays are world-major:
 * [n_worlds][n_bodies] and [n_worlds][n_tracers] rows, pos / vel interleaved x,y.  Every step advances the bodies and the
 * tracers of all worlds in at most two launches (one for the bodies, one for the tracers); there is no host synchronisation
 * between the steps of a call and nothing is read back.
 *   Bodies.  Every world's bodies take the step of nbody_ensemble_update_f32, from the same kernel and launch: they are
 *     bit-identical to an nbody_ensemble holding the same worlds, under EXACT, FAST and AUTO, with or without tracers.  With
 *     n_tracers == 0 the handle is an nbody_ensemble under another name.
 *   Tracers.  A tracer's acceleration is the field of its own world's bodies at their pre-step positions (the buffer that
 *     step's launch of the bodies reads): a_t = sum_j calculate_gravity(p_t, p_j, w_j), j ascending.  It has no mass and no self
 *     term (a tracer on a body meets that body's pair like any other).  It integrates as main.rs:419-423 in f32: v += a*dt;
 *     x += v*dt, multiply then add, no contraction.  Tracer rows never move.
 *   EXACT.  One ascending-row chain of the pair as written (IEEE divisions, the is_normal skip, no contraction) per tracer:
 *     bit-identical to the CPU restatement's direct_accel at the tracers (native accumulation) followed by that Euler step, and
 *     to a context of that world alone with the tracers of nbody_tracers_* under EXACT.
 *   FAST.  One lane per tracer, whatever n_bodies is.  The order of additions is the one the ensemble's bodies have for
 *     n_bodies > 128: source couples ascending, even and odd sources summed apart in a packed accumulator, every run of 64
 *     couples folded and added to the running total — a function of n_bodies alone, with the ensemble's pair (one v_rcp_f32,
 *     the 2^-90 biased denominator, s = m * rcp).  Hence every tracer is within the tolerance of DESIGN.md (2e-5 of
 *     sum_j |term|; worst case 6e-6 at n_bodies = 4096, as for the bodies), and for n_bodies > 128 a tracer that sits exactly
 *     on a body gets that body's FAST acceleration bit for bit (the self pair adds exactly 0 on both sides).
 *   AUTO.  Decided per world and per step on the device, without a flag buffer: a tracer block stages its whole world as a
 *     body block does, and a world whose bodies take EXACT for a step (a position outside FAST's domain: non-finite, >= 2^60 in
 *     magnitude, or non-zero below 2^-22) has all its tracers take EXACT for that step.  In a FAST world a tracer whose own
 *     pre-step position is outside that domain takes its EXACT value for that step; its neighbours keep their FAST bits.  With
 *     a clamp below 2^-19, or NaN, everything takes EXACT (FAST asked for by name, too).
 *   Independence.  A tracer's bits depend on its own state, its world's bodies, n_bodies and the params.  They do not depend on
 *     n_tracers, on its slot among the tracers, on n_worlds, on its world's index, on the other worlds' contents or routes, or
 *     on how the steps are split over calls.  For this the sources are never split over lanes, however few tracers a world has:
 *     a shape with few tracers per world leaves lanes idle (a block is 512 tracers of one world).
 *   Lifetime.  nbody_restricted_upload_f32 replaces the bodies and removes the tracers (a new world);
 *     nbody_restricted_tracers_upload_f32 replaces the tracers, n_tracers == 0 removes them (pos_xy / vel_xy may then be NULL);
 *     its n_worlds must be the bodies'.  Without tracers the tracer downloads and nbody_restricted_tracers_accel_f32 write
 *     nothing and return NBODY_OK.
 *   Booking, params, trivial calls.  As the ensemble's: the whole call goes under sum_gravity; clamp and arith are used;
 *     n_steps == 0 is a no-op; an update, accel or download before an upload is NBODY_ERR_INVALID.
 *   Errors.  Anything outside the limits gives NBODY_ERR_INVALID before anything is allocated, and the message names
 *     "restricted".  There is no CPU path: nbody_restricted_create fails with NBODY_ERR_NO_DEVICE without a gfx950 device.  A
 *     NULL handle gives NBODY_ERR_INVALID (0 from nbody_restricted_num_worlds / _num_bodies / _num_tracers);
 *     nbody_restricted_last_error(NULL): the last failed nbody_restricted_create on this thread, in a slot of its own.
 *   Not offered on this handle: f64 (nbody_restricted64_* below is the double-precision sibling); worlds of different sizes
 *     or a per-world n_tracers on this handle (nbody_rr_* at the end of this file offers both); tree methods; several devices; asynchronous snapshots and delta streams
 *     on a copy stream (the synchronous streams are nbody_deltas_restricted and the frames nbody_frames_restricted, both at the
 *     end of this file); hipGraph replay.  The library reads no environment variable for any of this. */
typedef struct nbody_restricted nbody_restricted;
int nbody_restricted_create(nbody_restricted** out, int device_id);
void nbody_restricted_destroy(nbody_restricted* e);
const char* nbody_restricted_last_error(const nbody_restricted* e);
int nbody_restricted_set_params(nbody_restricted* e, const nbody_params* p);
int nbody_restricted_get_params(const nbody_restricted* e, nbody_params* out);
int nbody_restricted_upload_f32(nbody_restricted* e, int64_t n_worlds, int64_t n_bodies, const float* pos_xy, const float* vel_xy,
                                const uint32_t* weight);
int nbody_restricted_download_f32(nbody_restricted* e, float* pos_xy, float* vel_xy);         /* the bodies; either may be NULL */
int nbody_restricted_tracers_upload_f32(nbody_restricted* e, int64_t n_worlds, int64_t n_tracers, const float* pos_xy,
                                        const float* vel_xy);
int nbody_restricted_tracers_download_f32(nbody_restricted* e, float* pos_xy, float* vel_xy); /* either may be NULL */
int64_t nbody_restricted_num_worlds(const nbody_restricted* e);
int64_t nbody_restricted_num_bodies(const nbody_restricted* e);                               /* per world */
int64_t nbody_restricted_num_tracers(const nbody_restricted* e);                              /* per world */
int nbody_restricted_update_f32(nbody_restricted* e, float delta, int n_steps, nbody_counting* counter);
int nbody_restricted_accel_f32(nbody_restricted* e, float* acc_xy);                           /* the bodies; state untouched */
int nbody_restricted_tracers_accel_f32(nbody_restricted* e, float* acc_xy);                   /* the tracers; state untouched */

/* ---- restricted ensembles in f64: double-precision tracers that step with each world, a handle of its own --------
 * The restricted ensemble above in double precision — test particles that run for many orbits around a few massive bodies, where
 * f32's 2^-24 per step is the error budget, not the force law.  Arrays, limits (1 <= n_bodies <= 4096, n_worlds * n_bodies <=
 * 2^26, n_tracers >= 0 and the same for every world, n_worlds * n_tracers <= 2^26), the two launches per step, lifetime, booking,
 * params, trivial calls and errors are as stated there, the messages naming "restricted"; no CPU path
 * (nbody_restricted64_create fails with NBODY_ERR_NO_DEVICE without a gfx950 device); NULL handle (NBODY_ERR_INVALID; 0 from
 * nbody_restricted64_num_worlds / _num_bodies / _num_tracers; nbody_restricted64_last_error(NULL): the last failed
 * nbody_restricted64_create on this thread — a slot of its own, apart from nbody_restricted_*'s and nbody_ensemble64_*'s).
 *   Bodies.  Every world's bodies take the step of nbody_ensemble64_update, from the same kernel and launch: they are
 *     bit-identical to an nbody_ensemble64 holding the same worlds, under every arith, with or without tracers.
 *   Tracers.  a_t = sum_j calculate_gravity(p_t, p_j, w_j as f64) over the bodies of the tracer's own world at their pre-step
 *     positions, j ascending, the pair of main.rs:234-253 in T = double with the clamp params.clamp widened to double; no mass
 *     and no self term; then main.rs:419-423 in double, multiply then add, no contraction.  Tracer rows never move.
 *   EXACT and AUTO.  One ascending-row chain of IEEE additions per tracer (two correctly rounded divisions per pair, the
 *     is_normal skip): bit-identical to the CPU restatement's direct_accel at the tracers (native accumulation) on float64
 *     followed by that Euler step, and to an f64 context of that world alone with the tracers of nbody_tracers_upload_f64 under
 *     EXACT.  AUTO is EXACT, as it is for nbody_ensemble64_* and for an f64 context.
 *   FAST (opt-in).  |a - a_ref|_1 <= 1e-12 * sum_j |term_j|_1 per tracer: v_rcp_f64 plus one Newton step, fused
 *     multiply-adds, the 2^-700 biased denominator.  One lane per tracer, whatever n_bodies is: the order of additions is the
 *     one nbody_ensemble64_*'s bodies have for n_bodies > 128 (runs of 64 sources, two fma chains per run, the runs added in
 *     order) — a function of n_bodies alone; for n_bodies > 128 a tracer that sits exactly on a body gets that body's FAST
 *     acceleration bit for bit.  Routed per world and per step on the device, without a flag buffer: a world with a body
 *     position outside the f64 FAST domain (non-finite, >= 2^100 in magnitude, or non-zero below 2^-300) at the start of a step
 *     has its bodies and all its tracers take EXACT for that step.  In a FAST world a tracer whose own pre-step position is
 *     outside that domain takes its EXACT value for that step; its neighbours keep their FAST bits.  With a clamp that is not
 *     > 0, or NaN, everything takes EXACT.
 *   Independence.  A tracer's bits depend on its own state, its world's bodies, n_bodies and the params — not on n_tracers, its
 *     slot, n_worlds, its world's index, the other worlds, or how the steps are split over calls.
 *   Staging.  A tracer block stages its world as a body block does: 80 KB of LDS at n_bodies = 4096 and no other LDS.
 *   Not offered on this handle: worlds of different sizes or a per-world n_tracers, tracers on several devices, and what the
 *     restricted ensemble above does not offer either. */
typedef struct nbody_restricted64 nbody_restricted64;
int nbody_restricted64_create(nbody_restricted64** out, int device_id);
void nbody_restricted64_destroy(nbody_restricted64* e);
const char* nbody_restricted64_last_error(const nbody_restricted64* e);
int nbody_restricted64_set_params(nbody_restricted64* e, const nbody_params* p);
int nbody_restricted64_get_params(const nbody_restricted64* e, nbody_params* out);
int nbody_restricted64_upload(nbody_restricted64* e, int64_t n_worlds, int64_t n_bodies, const double* pos_xy, const double* vel_xy,
                              const uint32_t* weight);
int nbody_restricted64_download(nbody_restricted64* e, double* pos_xy, double* vel_xy);         /* the bodies; either may be NULL */
int nbody_restricted64_tracers_upload(nbody_restricted64* e, int64_t n_worlds, int64_t n_tracers, const double* pos_xy,
                                      const double* vel_xy);
int nbody_restricted64_tracers_download(nbody_restricted64* e, double* pos_xy, double* vel_xy); /* either may be NULL */
int64_t nbody_restricted64_num_worlds(const nbody_restricted64* e);
int64_t nbody_restricted64_num_bodies(const nbody_restricted64* e);                             /* per world */
int64_t nbody_restricted64_num_tracers(const nbody_restricted64* e);                            /* per world */
int nbody_restricted64_update(nbody_restricted64* e, double delta, int n_steps, nbody_counting* counter);
int nbody_restricted64_accel(nbody_restricted64* e, double* acc_xy);                            /* the bodies; state untouched */
int nbody_restricted64_tracers_accel(nbody_restricted64* e, double* acc_xy);                    /* the tracers; state untouched */

/* ---- ragged restricted ensembles: worlds of different sizes, each with tracers of its own, a handle of its own (f32) ----
 * A stability map over systems with different numbers of massive bodies, capture cross-sections where each system gets as many
 * test particles as its own geometry needs, halos cut out of a larger run with their own tracer populations: the restricted
 * problem over worlds that differ in size AND in their number of tracers.  One nbody_restricted per distinct (n_bodies,
 * n_tracers) is one launch chain per shape again, and padding is wrong for the reason the ragged ensemble gives (a padded body
 * moves EXACT's chain and FAST's order of additions).  A ragged restricted ensemble holds n_worlds worlds of n_bodies[k] bodies
 * and n_tracers[k] massless points each and steps all of them with at most NBODY_RR_MAX_LAUNCHES launches per step.
 *   The prefix.  The calls are nbody_rr_* ("ragged restricted"), not nbody_ragged_restricted_* or nbody_restricted_ragged_*: the
 *     names that begin with nbody_ragged_ and with nbody_restricted_ are closed sets that belong to those two handles, and a
 *     handle of its own has a prefix that is a prefix of no other's.
 *   Arrays.  Body rows as nbody_ragged_*: world after world in world order, no padding, world k's rows [off_k, off_k + n_k).
 *     Tracer rows are laid out the same way: world k's tracers are the rows [toff_k, toff_k + m_k) with toff_k the sum of the
 *     counts before it; a world with m_k == 0 has none.  pos / vel interleaved x,y; weight may be NULL (all 1).
 *   Limits.  n_worlds >= 1, 1 <= n_bodies[k] <= 4096, the sizes add up to at most 2^26 rows; every n_tracers[k] >= 0, the counts
 *     add up to at most 2^26 rows.  Anything outside gives NBODY_ERR_INVALID before anything is allocated, and the message names
 *     "ragged restricted".  A refused upload leaves the bodies and the tracers as they were.
 *   Bodies.  They are bit-identical to an nbody_ragged holding the same worlds: they come from the same kernel and the same
 *     launches, under EXACT, FAST and AUTO, with or without tracers.
 *   Tracers.  A tracer's acceleration is the field of its own world's bodies at their pre-step positions (the buffer that
 *     step's launches of the bodies read): a_t = sum_j calculate_gravity(p_t, p_j, w_j), j ascending; no mass, no self term;
 *     then main.rs:419-423 in f32, multiply then add, no contraction.  Tracer rows never move.
 *   Tracers, EXACT.  They are bit-identical to the CPU restatement's direct_accel at the tracers (native accumulation) followed
 *     by the Euler step of main.rs:419-423.
 *   Tracers, FAST.  They are bit-identical to an nbody_restricted holding that world alone with those tracers: the two kernels
 *     share one block body, and the order of additions is a function of n_bodies[k] alone (one lane per tracer, whatever
 *     n_bodies[k] and n_tracers[k] are).  Hence every tracer is within the tolerance of DESIGN.md (2e-5 of sum_j |term|).
 *   AUTO.  The route is taken per world and per step on the device, from the staging block's OR over the world's body positions
 *     (outside FAST's domain: non-finite, >= 2^60 in magnitude, or non-zero below 2^-22), with no flag buffer: the same decision
 *     in every body block and every tracer block of the world.  The per-tracer exception is nbody_restricted_*'s: in a FAST world
 *     a tracer whose own pre-step position is outside that domain takes its EXACT value, its neighbours keep their FAST bits.  A
 *     clamp below 2^-19, or NaN, sends everything to EXACT (FAST asked for by name, too).
 *   Independence.  A tracer's bits depend on its own state, its world's bodies, n_bodies[k] and the params.  They do not depend
 *     on n_tracers[k]; on the tracer's slot; on the other worlds' sizes, counts, contents, routes or order; on the launch it
 *     falls in; or on how the steps are split over calls.
 *   Launches.  A step runs the bodies' launches of nbody_ragged_plan (at most 6, unchanged) and then the tracers' (at most 6);
 *     there is no host synchronisation between the steps of a call and nothing is read back.  Tracer blocks are grouped by the
 *     LDS their world needs, the six classes of the ragged ensemble (n_bodies <= 128, <= 256, ... <= 4096).  A class launches only
 *     if one of its worlds has tracers, under the LDS of the largest n_bodies among its worlds that have tracers.  World k
 *     contributes ceil(n_tracers[k] / 512) blocks (a block is up to 512 tracers of one world), contiguous, and within a launch
 *     the worlds follow one another in world order.  nbody_rr_plan shows this plan: for every world its launch and the first of
 *     its blocks in that launch — both -1 for a world without tracers, a convention of this call (nbody_ragged_plan has no world
 *     without a launch) — the number of launches (0 when no world has tracers), and per launch (arrays of
 *     NBODY_RAGGED_MAX_LAUNCHES, zero past n_launches) the dynamic LDS and the number of blocks.  It is pure host code: no device,
 *     no handle, every output pointer may be NULL; sizes or counts outside the limits give NBODY_ERR_INVALID and nothing is
 *     written.  The bodies' plan is nbody_ragged_plan of the sizes, unchanged.
 *   Lifetime.  nbody_rr_upload_f32 replaces the bodies and removes the tracers (new worlds).  nbody_rr_tracers_upload_f32
 *     replaces the tracers; its n_worlds must be the bodies'; an all-zero n_tracers removes them (pos_xy / vel_xy may then be
 *     NULL).  Without tracers the tracer downloads and nbody_rr_tracers_accel_f32 write nothing and return NBODY_OK.
 *     nbody_rr_sizes writes the sizes and the counts (zeros without tracers); either output may be NULL.
 *   Booking, params, trivial calls.  As the ensemble's: the whole call goes under sum_gravity; clamp and arith are used;
 *     n_steps == 0 is a no-op; an update, accel or download before an upload is NBODY_ERR_INVALID.
 *   Errors.  There is no CPU path: nbody_rr_create fails with NBODY_ERR_NO_DEVICE without a gfx950 device.  A NULL handle gives
 *     NBODY_ERR_INVALID (0 from nbody_rr_num_worlds / _num_rows / _num_tracer_rows); nbody_rr_last_error(NULL): the last failed
 *     nbody_rr_create or nbody_rr_plan on this thread, in a slot of its own.
 *   Not offered on this handle: f64 (nbody_rr64_* below is the double-precision sibling); tree methods; several
 *     devices; asynchronous snapshots and delta streams on a copy stream (the synchronous streams are nbody_deltas_rr and the
 *     frames nbody_frames_rr, both at the end of this file); hipGraph replay.  The library reads no environment variable for any
 *     of this. */
#define NBODY_RR_MAX_LAUNCHES 12
typedef struct nbody_rr nbody_rr;
int nbody_rr_create(nbody_rr** out, int device_id);
void nbody_rr_destroy(nbody_rr* e);
const char* nbody_rr_last_error(const nbody_rr* e);
int nbody_rr_set_params(nbody_rr* e, const nbody_params* p);
int nbody_rr_get_params(const nbody_rr* e, nbody_params* out);
int nbody_rr_upload_f32(nbody_rr* e, int64_t n_worlds, const int64_t* n_bodies /*[n_worlds]*/, const float* pos_xy,
                        const float* vel_xy, const uint32_t* weight);
int nbody_rr_download_f32(nbody_rr* e, float* pos_xy, float* vel_xy);             /* the bodies; either may be NULL */
int nbody_rr_tracers_upload_f32(nbody_rr* e, int64_t n_worlds, const int64_t* n_tracers /*[n_worlds]*/, const float* pos_xy,
                                const float* vel_xy);
int nbody_rr_tracers_download_f32(nbody_rr* e, float* pos_xy, float* vel_xy);     /* either may be NULL */
int64_t nbody_rr_num_worlds(const nbody_rr* e);
int64_t nbody_rr_num_rows(const nbody_rr* e);                                     /* the sum of the sizes */
int64_t nbody_rr_num_tracer_rows(const nbody_rr* e);                              /* the sum of the tracer counts */
int nbody_rr_sizes(const nbody_rr* e, int64_t* n_bodies_out /*[num_worlds]*/, int64_t* n_tracers_out /*[num_worlds]*/);
int nbody_rr_update_f32(nbody_rr* e, float delta, int n_steps, nbody_counting* counter);
int nbody_rr_accel_f32(nbody_rr* e, float* acc_xy);                               /* the bodies; state untouched */
int nbody_rr_tracers_accel_f32(nbody_rr* e, float* acc_xy);                       /* the tracers; state untouched */
int nbody_rr_plan(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, int32_t* launch_of_world,
                  int64_t* first_block_of_world, int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch);

/* ---- ragged restricted ensembles in f64: double-precision worlds of different sizes, each with tracers of its own --------
 * The ragged restricted ensemble above in double precision: n_worlds worlds of n_bodies[k] bodies and n_tracers[k] massless
 * points each, float64 arrays, stepped with at most NBODY_RR_MAX_LAUNCHES launches per step (the constant serves both
 * precisions).  One nbody_restricted64 per distinct (n_bodies, n_tracers) is one launch chain per shape; this handle is one.
 *   The prefix.  The calls are nbody_rr64_*, typed calls without a suffix as the other f64 handles name theirs.  The prefix
 *     begins with none of nbody_rr_, nbody_ragged64_ or nbody_restricted64_: those are closed sets of their own handles.
 *   Arrays.  As nbody_rr_*, in double: body rows world after world in world order, no padding, world k's rows [off_k, off_k +
 *     n_k); tracer rows the same way, world k's tracers the rows [toff_k, toff_k + m_k), none for m_k == 0.  pos / vel
 *     interleaved x,y; weight may be NULL (all 1); the masses are the u32 weights (`weight as f64` is exact).
 *   Limits.  n_worlds >= 1, 1 <= n_bodies[k] <= 4096, the sizes add up to at most 2^26 rows; every n_tracers[k] >= 0, the counts
 *     add up to at most 2^26 rows.  Anything outside gives NBODY_ERR_INVALID before anything is allocated, and the message names
 *     "ragged restricted".  A refused upload leaves the bodies and the tracers as they were.
 *   Bodies.  They are bit-identical to an nbody_ragged64 holding the same worlds: the same kernel and the same launches, under
 *     every arith, with or without tracers.
 *   Tracers.  a_t = sum_j calculate_gravity(p_t, p_j, w_j as f64) over the bodies of the tracer's own world at their pre-step
 *     positions (the buffer that step's launches of the bodies read), j ascending, the clamp params.clamp widened to double; no
 *     mass, no self term; then main.rs:419-423 in double, multiply then add, no contraction.  Tracer rows never move.
 *   Tracers, EXACT and AUTO.  AUTO is EXACT, as for every f64 handle.  One ascending-row chain of IEEE additions per tracer:
 *     bit-identical to the CPU restatement's direct_accel at the tracers (native accumulation) on float64 followed by that Euler
 *     step: what nbody_restricted64_* promises.
 *   Tracers, FAST (opt-in).  They are bit-identical to an nbody_restricted64 holding that world alone with those tracers: the two
 *     kernels share one block body, and the order of additions is a function of n_bodies[k] alone (one lane per tracer, whatever
 *     n_bodies[k] and n_tracers[k] are).  Hence every tracer is within 1e-12 of sum_j |term_j|_1, and for
 *     n_bodies[k] > 128 a tracer that sits exactly on a body gets that body's FAST acceleration bit for bit.  The route is taken
 *     per world and per step on the device from the staging's OR over the world's body positions (outside the f64 FAST domain:
 *     non-finite, >= 2^100 in magnitude, or non-zero below 2^-300), with no flag buffer: the same decision in every body block
 *     and every tracer block of the world, and such a world's bodies and tracers take EXACT for that step.  In a FAST world a
 *     tracer whose own pre-step position is outside that domain takes its EXACT value; its neighbours keep their FAST bits.
 *     With a clamp that is not > 0, or NaN, everything takes EXACT.
 *   Independence.  A tracer's bits depend on its own state, its world's bodies, n_bodies[k] and the params.  They do not depend
 *     on n_tracers[k]; on the tracer's slot; on the other worlds' sizes, counts, contents, routes or order; on the launch it
 *     falls in; or on how the steps are split over calls.
 *   Launches.  A step runs the bodies' launches of nbody_ragged64_plan (at most 6, unchanged) and then the tracers' (at most 6),
 *     with no host synchronisation between the steps of a call.  The tracers' plan is nbody_rr_plan's under the f64 LDS function
 *     (20 bytes a body, the rows padded to a multiple of 8; 81 920 B at n_bodies = 4096 and no other LDS): the six classes by
 *     n_bodies, a class launching only if one of its worlds has tracers, under the LDS of the largest n_bodies among its worlds
 *     that have tracers; ceil(n_tracers[k] / 512) contiguous blocks per world, worlds in world order.  nbody_rr64_plan shows it,
 *     with the outputs and conventions of nbody_rr_plan (-1 / -1 for a world without tracers; pure host code; every output may
 *     be NULL; nothing is written on NBODY_ERR_INVALID).
 *   Lifetime.  nbody_rr64_upload replaces the bodies and removes the tracers (new worlds).  nbody_rr64_tracers_upload replaces
 *     the tracers; its n_worlds must be the bodies'; an all-zero n_tracers removes them (pos_xy / vel_xy may then be NULL).
 *     Without tracers the tracer downloads and nbody_rr64_tracers_accel write nothing and return NBODY_OK.  nbody_rr64_sizes
 *     writes the sizes and the counts (zeros without tracers); either output may be NULL.
 *   Booking, params, trivial calls.  As the ensemble's: the whole call goes under sum_gravity; clamp and arith are used;
 *     n_steps == 0 is a no-op; an update, accel or download before an upload is NBODY_ERR_INVALID.
 *   Errors.  There is no CPU path: nbody_rr64_create fails with NBODY_ERR_NO_DEVICE without a gfx950 device.  A NULL handle
 *     gives NBODY_ERR_INVALID (0 from nbody_rr64_num_worlds / _num_rows / _num_tracer_rows); nbody_rr64_last_error(NULL): the
 *     last failed nbody_rr64_create or nbody_rr64_plan on this thread, in a slot of its own, apart from nbody_rr_*'s and
 *     nbody_ragged64_*'s.
 *   Not offered on this handle: what nbody_rr_* does not offer either. */
typedef struct nbody_rr64 nbody_rr64;
int nbody_rr64_create(nbody_rr64** out, int device_id);
void nbody_rr64_destroy(nbody_rr64* e);
const char* nbody_rr64_last_error(const nbody_rr64* e);
int nbody_rr64_set_params(nbody_rr64* e, const nbody_params* p);
int nbody_rr64_get_params(const nbody_rr64* e, nbody_params* out);
int nbody_rr64_upload(nbody_rr64* e, int64_t n_worlds, const int64_t* n_bodies /*[n_worlds]*/, const double* pos_xy,
                      const double* vel_xy, const uint32_t* weight);
int nbody_rr64_download(nbody_rr64* e, double* pos_xy, double* vel_xy);           /* the bodies; either may be NULL */
int nbody_rr64_tracers_upload(nbody_rr64* e, int64_t n_worlds, const int64_t* n_tracers /*[n_worlds]*/, const double* pos_xy,
                              const double* vel_xy);
int nbody_rr64_tracers_download(nbody_rr64* e, double* pos_xy, double* vel_xy);   /* either may be NULL */
int64_t nbody_rr64_num_worlds(const nbody_rr64* e);
int64_t nbody_rr64_num_rows(const nbody_rr64* e);                                 /* the sum of the sizes */
int64_t nbody_rr64_num_tracer_rows(const nbody_rr64* e);                          /* the sum of the tracer counts */
int nbody_rr64_sizes(const nbody_rr64* e, int64_t* n_bodies_out /*[num_worlds]*/, int64_t* n_tracers_out /*[num_worlds]*/);
int nbody_rr64_update(nbody_rr64* e, double delta, int n_steps, nbody_counting* counter);
int nbody_rr64_accel(nbody_rr64* e, double* acc_xy);                              /* the bodies; state untouched */
int nbody_rr64_tracers_accel(nbody_rr64* e, double* acc_xy);                      /* the tracers; state untouched */
int nbody_rr64_plan(int64_t n_worlds, const int64_t* n_bodies, const int64_t* n_tracers, int32_t* launch_of_world,
                    int64_t* first_block_of_world, int32_t* n_launches, int32_t* lds_bytes_of_launch, int64_t* blocks_of_launch);

/* ---- frames of an ensemble: every world's draw() raster from one call ---------------------------------------------
 * The hand-off of a viewer (World::update feeds draw()) for all eight handles above: a contact sheet of the worlds without
 * downloading their rows and without one context per world.  World k's tile is the reference's draw() (main.rs:41-72) of its
 * own rows alone, byte for byte what nbody_render_rgba gives for a context holding that world: its bodies in upload order
 * (ensemble rows never move) and then, where with_tracers != 0, its tracers in upload order as rows n .. n+m-1 of weight 1.
 *   The prefix.  nbody_frames_<handle>: the names under each handle's own prefix are closed sets, so these calls have a prefix
 *     of their own, followed by the handle's name.
 *   Output.  rgba_out is host memory, [n_worlds][render_px][render_px][4] bytes, R G B A.  Per pixel of a world: a row of
 *     weight > 10 makes it (0,255,0,255); otherwise with c light rows on it, the last of them in row order having
 *     v = 0x10 + min(((|vx|+|vy|)*10) as u8, 0xef), it is (255, 255-v, 255-v, min(10 c, 250)); without a row it is 0.  Rows
 *     outside [0, height)^2, and rows with a NaN position, touch nothing.
 *   Calls.  Synchronous, on the handle's stream.  They read the current positions and write nothing of the state: stepping
 *     with frames in between gives the bits of stepping alone.  The device scratch (the tiles, the work words, a ragged
 *     handle's table of row ranges) belongs to the handle, is grown on demand and is freed with its other arrays.
 *   Tracers.  with_tracers != 0 on a handle that holds no tracers gives the bodies' frames; in the nbody_rr handles a world
 *     with no tracers is painted from its bodies.
 *   Routes.  Chosen by render_px alone.  render_px <= 101 (render_px^2 * 8 <= 81 920 bytes of LDS): one launch, one block per
 *     world, the world's pixels accumulated in LDS.  Above: a zeroed work buffer, one launch over the rows of all worlds, one over
 *     their pixels.  The bytes are the same.  Where the two cross over in time has not been measured; profiles/
 *     ensemble_frames.txt records both at neighbouring sizes.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or launched, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "frames": nothing uploaded; rgba_out NULL; height or
 *     render_px 0; render_px not dividing height, or height > 2^24 (as nbody_render_rgba refuses them); n_worlds * render_px^2 >
 *     2^26 pixels; a world whose bodies and tracers together are more than 2^24 rows when tracers are asked for (the message
 *     names "tracers").  A NULL handle gives NBODY_ERR_INVALID without a message.
 *   Not offered: a device-pointer variant; the contact sheet itself (tile the frames on the host); snapshots (the delta
 *     streams of an ensemble are nbody_deltas_* below). */
int nbody_frames_ensemble(nbody_ensemble* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out);
int nbody_frames_ensemble64(nbody_ensemble64* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out);
int nbody_frames_ragged(nbody_ragged* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out);
int nbody_frames_ragged64(nbody_ragged64* e, uint32_t height, uint32_t render_px, uint8_t* rgba_out);
int nbody_frames_restricted(nbody_restricted* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out);
int nbody_frames_restricted64(nbody_restricted64* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out);
int nbody_frames_rr(nbody_rr* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out);
int nbody_frames_rr64(nbody_rr64* e, uint32_t height, uint32_t render_px, int with_tracers, uint8_t* rgba_out);

/* ---- delta streams of an ensemble: every world's NBD1 stream from one call ---------------------------------------
 * The recording hand-off for all eight handles above: one lossless delta stream per world (the format "NBD1" of
 * nbody_delta_begin / nbody_delta_end, decoded by nbody_delta_decoder_*, one decoder per world), about a byte per body and step
 * where the raw rows are 8 or 16, without one context per world.  A segment is one world's bodies or one world's tracers: n rows
 * in upload order (ensemble rows never move: no ids, no scatter).
 *   The prefix.  nbody_deltas_<handle> — with the s: the names under each handle's own prefix, under nbody_frames_ and under
 *     nbody_delta_ are closed sets.
 *   Per-world bytes.  Every segment's stream is byte for byte what a context holding that world alone returns from
 *     nbody_delta_begin / nbody_delta_end (for tracers: nbody_tracers_delta_*) at the same step count after the same resets:
 *     header (NBD1, element bits 32 | 64, key flag, n, step, payload words), width bytes zero padded to a multiple of 8, the
 *     bit-plane payload with the predictor chosen per (64-row block, coordinate), ties to predictor 0, lanes past n holding z = 0.
 *     A segment of 0 rows is its 32-byte header alone: a world of an nbody_rr handle without tracers, every world of a restricted
 *     handle when tracers are asked for while it holds none.
 *   Independence.  A segment's bytes depend only on its own position history, the step numbers and the resets; not on the number
 *     of worlds, its index, the other worlds' sizes or contents, or the launch it falls in.
 *   Step.  The handle counts the steps it has taken since it was created; the count runs on across uploads, as a context's
 *     does.  It is written to every header of the call and to *step_out (which may be NULL).
 *   Sequences.  A handle keeps one sequence for the bodies and one for the tracers (NBODY_DELTAS_TRACERS addresses the latter),
 *     each with the keys of its last two streams.  The first stream after an upload of bodies is a key frame; an upload of bodies
 *     removes the tracers and so resets both sequences; an upload of tracers resets the tracers' sequence only.  The bodies'
 *     streams are the same bytes with or without tracers, and whether or not tracer streams are taken.  NBODY_DELTAS_KEY makes
 *     this call's streams key frames of the sequence it addresses.
 *   Read-only.  The call reads the current positions and writes no simulation state: stepping with these calls in between
 *     gives the bits of stepping alone.
 *   Commit.  The sequence advances only when the streams have been copied out; a refused call changes nothing.  With cap smaller
 *     than the streams (out may then be NULL with cap == 0: a question for the size) the call writes *bytes_out = the bytes
 *     needed, returns NBODY_ERR_INVALID with a message that contains "smaller than the stream", and the same call with a larger
 *     buffer returns the bytes the first would have returned.
 *   Output.  The streams one after another in world order in out[0, *bytes_out); every stream's size is a multiple of 8, so
 *     every stream starts 8-aligned.  offsets_out (may be NULL): [n_worlds + 1], the byte offset of every world's stream and then
 *     the total.  Synchronous, on the handle's stream; a fixed number of launches, whatever the number of worlds.  The device
 *     scratch belongs to the handle, is made by the first call after an upload and freed with the rows it describes.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or launched, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "deltas": nothing uploaded; out NULL with cap != 0;
 *     bytes_out NULL; unknown flag bits; NBODY_DELTAS_TRACERS on one of the four handles that have no tracer calls; more than 2^24
 *     blocks of 64 rows in the addressed segments, sum_k ceil(n_k / 64) > 2^24 (the payload is addressed in 32-bit words).  A
 *     NULL handle gives NBODY_ERR_INVALID without a message.
 *   nbody_deltas_bound.  Pure host code: the sum of nbody_delta_bound(rows[k], is_f64), the largest the streams of these
 *     segments can be; 0 for a NULL or negative argument and for more than 2^24 blocks.
 *   Not offered: snapshots of an ensemble (the calls are synchronous and *_download* hands the rows out whole; an ensemble has no
 *     copy stream to run under the next step); a device-pointer variant; a per-world reset. */
#define NBODY_DELTAS_TRACERS 1u /* the tracers' sequence, not the bodies' */
#define NBODY_DELTAS_KEY 2u     /* make this a key frame */
int nbody_deltas_ensemble(nbody_ensemble* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                          uint64_t* step_out);
int nbody_deltas_ensemble64(nbody_ensemble64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                            uint64_t* step_out);
int nbody_deltas_ragged(nbody_ragged* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                        uint64_t* step_out);
int nbody_deltas_ragged64(nbody_ragged64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                          uint64_t* step_out);
int nbody_deltas_restricted(nbody_restricted* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                            uint64_t* step_out);
int nbody_deltas_restricted64(nbody_restricted64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out,
                              uint64_t* offsets_out, uint64_t* step_out);
int nbody_deltas_rr(nbody_rr* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                    uint64_t* step_out);
int nbody_deltas_rr64(nbody_rr64* e, uint32_t flags, uint8_t* out, size_t cap, size_t* bytes_out, uint64_t* offsets_out,
                      uint64_t* step_out);
size_t nbody_deltas_bound(int64_t n_segments, const int64_t* rows /*[n_segments], each >= 0*/, int is_f64);

/* ---- sweeps of an ensemble: a time step, a clamp and a number of steps per world ---------------------------------
 * What the ensembles are for — a time-step convergence study, a softening sweep — for all eight handles above: *_update steps
 * every world by one delta under one params.clamp, so a study over either was one handle per value again.  A sweep is an update
 * in which world k steps by delta[k] under clamp[k] and takes steps[k] steps: a convergence study steps world k with delta_k =
 * T / steps_k, so the worlds need different step counts to reach the same end time.
 *   The prefix.  nbody_sweep_<handle>: the names under each handle's own prefix, under nbody_frames_ and under nbody_deltas_
 *     are closed sets, so these eight have a prefix of their own.
 *   Arguments.  delta, clamp and steps are host arrays of n_worlds elements, read during the call only.  The call is stateless:
 *     nothing of a sweep stays in the handle (params are neither read back nor changed), so uploads, set_params, frames and
 *     delta streams need no new rule.
 *       delta[k]   required.  World k's time step, used as *_update's delta is (v += a*dt; x += v*dt, multiply then add, no
 *                  contraction).  Any value is taken, as *_update takes any.  double on the f64 handles.
 *       clamp[k]   may be NULL: every world uses params.clamp.  float on all eight handles, as params.clamp is; widened to double
 *                  on the f64 handles.
 *       steps[k]   may be NULL: every world takes n_steps steps.  World k takes the first steps[k] of the call's n_steps steps and
 *                  then stands still: its positions and velocities (and its tracers') keep their bits exactly, whatever they are
 *                  (-0.0, NaN payloads, infinities).  0 <= steps[k] <= n_steps.
 *   Per-world contract.  World k's bits are those of a handle of the same kind holding world k alone, with params.clamp =
 *     clamp[k], stepped by *_update(delta[k], steps[k]) — under the handle's arith, for bodies and tracers.  So the handles'
 *     promises carry over world by world: EXACT is bit-identical to the CPU restatement's update_direct of that world with its
 *     own delta, clamp and nsteps (tracers: its direct_accel at the tracers plus the Euler step); FAST and AUTO are bit-identical
 *     to that world alone on the same kind of handle.
 *   Independence.  As every handle states it, and: a world's bits do not depend on the other worlds' delta, clamp or steps, nor
 *     on n_steps beyond steps[k], nor on how a sweep is split over calls (steps split accordingly).
 *   Route.  The tests that turn a whole handle EXACT for its clamp are taken per world, on the device, by the blocks of that
 *     world: on the f32 handles a world whose clamp[k] is below 2^-19, or NaN, takes EXACT for the call (under AUTO, and under
 *     FAST asked for by name); on the f64 handles a world takes FAST only under arith FAST with clamp[k] > 0.  Its neighbours keep
 *     their FAST bits.  With clamp given, params.clamp decides nothing.  arith EXACT sends every world to EXACT; the per-step
 *     decision of AUTO on a world's positions and the per-tracer exception in a FAST world are what they were.
 *   Calls.  Synchronous: n_steps steps enqueued back to back on the handle's stream, one synchronisation at the end, nothing
 *     read back in between.  The launches per step are those of *_update (1; 2 with tracers; at most 6 ragged; at most 12 ragged
 *     restricted), whatever steps[] holds.  The seconds are booked under sum_gravity, as *_update books them.
 *   Step count.  The handle's count of steps (nbody_deltas_*) advances by n_steps: it counts the handle's launches.  A world's
 *     stream header after a sweep therefore carries the handle's count, not the number of steps that world has itself taken.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or enqueued, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "sweep": nothing uploaded; delta NULL; n_steps < 0; a
 *     steps[k] outside [0, n_steps] (the message names the world).  n_steps == 0 after those checks is a no-op.  A NULL handle
 *     gives NBODY_ERR_INVALID without a message.
 *   Not offered: a per-world arith; per-world parameters for *_accel (it keeps params.clamp); a device-pointer variant; hipGraph
 *     replay of a sweep; anything for nbody_ctx contexts. */
int nbody_sweep_ensemble(nbody_ensemble* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                         nbody_counting* counter);
int nbody_sweep_ensemble64(nbody_ensemble64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                           nbody_counting* counter);
int nbody_sweep_ragged(nbody_ragged* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                       nbody_counting* counter);
int nbody_sweep_ragged64(nbody_ragged64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                         nbody_counting* counter);
int nbody_sweep_restricted(nbody_restricted* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps,
                           nbody_counting* counter);
int nbody_sweep_restricted64(nbody_restricted64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                             nbody_counting* counter);
int nbody_sweep_rr(nbody_rr* e, const float* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter);
int nbody_sweep_rr64(nbody_rr64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps,
                     nbody_counting* counter);

/* ---- summaries of an ensemble: per-world moments, extent and separations from one call ---------------------------
 * What a study over many worlds ends in, for all eight handles above, without a download of all rows and a host loop: a
 * convergence study wants how far world k is from the finest world, a seed ensemble how fast neighbouring trajectories separate,
 * a stability map how many tracers of each world are still inside the frame, and anyone watching a long run the centre of mass,
 * the momentum, the kinetic sum, the extent and whether anything went non-finite.  A segment is one world's bodies or one
 * world's tracers (NBODY_SUMMARY_TRACERS); its record is a function of its own rows — and, for the separation, of the rows of
 * the world ref[k] names — bit for bit, whatever the number of worlds, the world's index or the other worlds hold.
 *   The prefix.  nbody_summary_<handle>, and nbody_summary_of_f32 / _of_f64: the names under each handle's own prefix, under
 *     nbody_frames_, nbody_deltas_ and nbody_sweep_ are closed sets, so these ten have a prefix of their own.
 *   Arithmetic.  Everything is double on all eight handles.  A row's x, y, vx, vy are widened to double (exact).  w is the
 *     double of what the handle holds: `weight as f32` on the f32 handles, the u32 weight on the f64 handles, 1 for a tracer.
 *     Every *, + and - written below is one IEEE double operation in the written grouping; nothing is fused.
 *   counted.  The rows whose x, y, vx, vy are all finite; only these enter the fields from mass to sum_wv2.
 *   mass.  The sum of w over counted rows: integers of at most 2^32 over at most 2^26 rows, exact, hence order-free.
 *   min_x, min_y, max_x, max_y, max_speed2.  Over counted rows, ordered by value with -0.0 below +0.0, hence order-free;
 *     max_speed2 is the largest vx*vx + vy*vy.  With counted == 0 the minima are +inf, the maxima -inf and max_speed2 +0.0.
 *   in_bounds.  The rows with y < H && x < H && y >= 0 && x >= 0 for H = height (within_bounds, main.rs:224-226), by position
 *     alone, counted or not: the rows draw() and nbody_frames_* would paint.  height == 0 gives 0.
 *   sum_wx, sum_wy, sum_wvx, sum_wvy, sum_wv2.  The sums over counted rows of w*x, w*y, w*vx, w*vy and w*(vx*vx + vy*vy): centre
 *     of mass = (sum_wx, sum_wy) / mass, momentum, twice the kinetic sum.
 *   Separation.  ref[k] = j >= 0 names a world of the same handle with the same number of rows in the addressed segment (ref[k]
 *     == k is allowed).  Every row r counted in both worlds gives dx = x_k - x_j, dy = y_k - y_j, d2 = dx*dx + dy*dy; sep_rows
 *     counts these rows, sep_max2 is the largest d2 and sep_sum2 their sum, d2 in row r's slot of the order below.  ref == NULL
 *     or ref[k] == -1 gives 0, +0.0 and +0.0.
 *   The order of the six sums (sum_wx .. sum_wv2, sep_sum2).  A function of the row index alone.  A segment is cut into chunks
 *     of 4096 rows.  In chunk c, chain l (0 <= l < 256) starts at +0.0 and adds the terms of rows 4096 c + l + 256 i for i = 0 ..
 *     15 ascending; a row past the end, or one that does not contribute, adds nothing.  Then for s = 128, 64, .., 1: P[l] = P[l] +
 *     P[l + s] for l < s, and the chunk's value is P[0].  The segment's value is chunk 0's value plus chunk 1's and so on,
 *     ascending.  Bodies are always one chunk.  A sum that overflows and turns into NaN is a NaN; its sign and payload are not
 *     promised (an x86 host and the device make different default NaNs).
 *   Calls.  Synchronous, on the handle's stream.  They read the current rows and write nothing of the state: stepping with
 *     summaries in between gives the bits of stepping alone.  One launch for the bodies; for the tracers one, and a second
 *     where a world has more than 4096 of them, whatever the number of worlds; no floating-point atomics; nothing is read
 *     back before the end.  The device scratch belongs to the handle,
 *     is grown on demand and is freed with its other arrays.  out: host memory, one record per world.
 *   Tracers.  NBODY_SUMMARY_TRACERS on a restricted handle that holds no tracers gives records with rows == 0 (counts 0, mass
 *     and sums +0.0, minima +inf, maxima -inf), as does a world of an nbody_rr handle without tracers.
 *   nbody_summary_of_f32 / _of_f64.  Pure host code, no device, no handle: one segment's record by the contract above — the CPU
 *     statement of it, the same bits.  weight NULL: every w is 1; for f32, w is `(double)(float)weight`.  ref_pos_xy NULL: no
 *     separation; with it ref_vel_xy is required (it says which reference rows are counted).  They refuse rows < 0, out NULL,
 *     NULL arrays with rows > 0, and a ref_pos_xy without a ref_vel_xy, with NBODY_ERR_INVALID and no message.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or launched, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "summary": nothing uploaded; out NULL; unknown flag
 *     bits; NBODY_SUMMARY_TRACERS on one of the four handles that have no tracer calls; height > 2^24; a ref[k] outside
 *     [-1, n_worlds) (the message names the world); on the ragged handles a ref[k] whose segment has another number of rows
 *     than world k's (the message names the world).  A NULL handle gives NBODY_ERR_INVALID without a message.
 *   Not offered: a velocity or phase-space separation; a potential energy (the reference's pair law, main.rs:234-253, is not the
 *     gradient of the Newtonian potential, so there is no energy this step conserves); a device-pointer variant; anything for
 *     nbody_ctx contexts. */
typedef struct nbody_world_summary { /* 17 fields of 8 bytes, no padding: 136 bytes */
  int64_t rows;      /* rows of the segment: the world's bodies, or its tracers */
  int64_t counted;   /* rows whose x, y, vx, vy are all finite; only these enter the fields from mass to sum_wv2 */
  int64_t in_bounds; /* rows whose position passes within_bounds (main.rs:224-226) under `height`, by position alone */
  int64_t sep_rows;  /* rows counted both here and in the reference world */
  double mass;       /* sum of w over counted rows */
  double min_x, min_y, max_x, max_y; /* over counted rows */
  double max_speed2; /* max over counted rows of vx*vx + vy*vy */
  double sum_wx, sum_wy;   /* centre of mass = these / mass */
  double sum_wvx, sum_wvy; /* momentum */
  double sum_wv2;    /* sum of w*(vx*vx + vy*vy): twice the kinetic sum */
  double sep_max2, sep_sum2; /* max and sum of squared distances to the reference world's rows */
} nbody_world_summary;
#define NBODY_SUMMARY_TRACERS 1u /* the tracers' segment, not the bodies' */
int nbody_summary_ensemble(nbody_ensemble* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                           nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_ensemble64(nbody_ensemble64* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                             nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_ragged(nbody_ragged* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                         nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_ragged64(nbody_ragged64* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                           nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_restricted(nbody_restricted* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                             nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_restricted64(nbody_restricted64* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                               nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_rr(nbody_rr* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                     nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_rr64(nbody_rr64* e, uint32_t flags, uint32_t height, const int32_t* ref /*[n_worlds] or NULL*/,
                       nbody_world_summary* out /*[n_worlds]*/);
int nbody_summary_of_f32(int64_t rows, const float* pos_xy, const float* vel_xy, const uint32_t* weight /*NULL: all 1*/,
                         const float* ref_pos_xy /*NULL: none*/, const float* ref_vel_xy, uint32_t height, nbody_world_summary* out);
int nbody_summary_of_f64(int64_t rows, const double* pos_xy, const double* vel_xy, const uint32_t* weight /*NULL: all 1*/,
                         const double* ref_pos_xy /*NULL: none*/, const double* ref_vel_xy, uint32_t height, nbody_world_summary* out);

/* ---- encounters of an ensemble: per target its nearest neighbour and its clamped pairs, per world one record --------
 * What a softening sweep asks — is the clamp deciding the result? — and what a restricted problem asks of every tracer — which
 * body is nearest, and how near (capture, impact, close fly-by) — for all eight handles above, without a download of all rows and
 * an O(n^2) loop per world on the host.  The pair law (calculate_gravity, main.rs:234-253) replaces `distance` by the clamp
 * wherever dx*dx + dy*dy < clamp, and drops a pair wherever |dx| + |dy| is not a normal number; no summary field shows either.
 * A segment's targets are one world's bodies or, with NBODY_ENCOUNTERS_TRACERS, one world's tracers; its sources are that
 * world's bodies.
 *   The prefix.  nbody_encounters_<handle>, and nbody_encounters_of_f32 / _of_f64: a closed set of ten, under a prefix of its own.
 *   Arithmetic.  The handle's own precision T (float on the f32 handles, double on the f64 ones), with exactly the step's
 *     expressions: dx = xj - xi, dy = yj - yi, sum = |dx| + |dy|, d2 = dx*dx + dy*dy.  Each operation is one IEEE operation in
 *     T; nothing is fused.  So d2 is the very `distance` the step compares with its clamp, under any params.arith: an encounter
 *     report does not depend on arith.
 *     Live.  A pair is live when `sum` is a normal number; otherwise it is skipped (coincident bodies, subnormal differences,
 *     non-finite rows).  A live d2 is never NaN or negative: it lies in [+0, +inf], and both ends occur — d2 can underflow to +0
 *     while `sum` is normal, and overflow to +inf while `sum` is finite.  Both are live pairs: an overflowed d2 = +inf comes with
 *     nn_index >= 0, "no live pair" with nn_index == -1 and nn_d2 = +inf.
 *     Close.  A pair is close when it is live and d2 < limit2[k] (widened to double on the f64 handles, as a step widens its
 *     clamp).  A NaN or zero limit gives no close pair; +inf makes every live pair with a finite d2 close.  limit2 == NULL:
 *     every world uses params.clamp, and close_pairs is then the number of ordered pairs whose force the clamp altered in a
 *     step from these rows.
 *   Fields.  Per target: nn_d2 is the smallest live d2, nn_index the world-local index of the source that attains it, close the
 *     target's number of close pairs.  Per world: the counts are integer sums over its targets; min_* is the smallest nn_d2 over
 *     the targets that have a neighbour, min_source that row's nn_index; max_nn_* the largest nn_d2 over the same targets.
 *     Both doubles are the T values widened (exact).
 *   Tie rules.  nn_index is the lowest source index that attains nn_d2; min_row and max_nn_row are the lowest row that attains
 *     the extreme.  With them every output is order-free — minima and maxima with an index rule, and integer counts — so the
 *     contract is bit for bit, without a tolerance, and the kernel is free to cut the sources into chunks: walking j ascending
 *     and replacing on a strict `<` gives the lowest index.
 *   Bodies.  The sources are the world's bodies; j == i is excluded by index, is not a pair and is counted nowhere.  A distinct
 *     coincident body is a skipped pair.  live_pairs + skipped_pairs == rows * (sources - 1).
 *   Tracers.  With NBODY_ENCOUNTERS_TRACERS the targets are the world's tracers and the sources all its bodies: live_pairs +
 *     skipped_pairs == rows * sources.  Tracer-tracer pairs do not exist (tracers are massless).  A restricted handle without
 *     tracers, or a world of an nbody_rr handle without them, gives rows == 0: zero counts, -1 indices, min_d2 = +inf.
 *     max_nn_d2 is +0.0 wherever no target has a neighbour.
 *   Layout.  nn_index, nn_d2 and close are host memory, one entry per target of all worlds, laid out as the handle's
 *     *_download (for the tracers: *_tracers_download) lays out that segment's rows; each may be NULL.  nn_d2 is float on the
 *     f32 handles and double on the f64 ones; limit2 is float on all eight, as a sweep's clamp is.
 *   Independence.  A world's record and rows are a function of its own rows and limit2[k] alone: not of the number of worlds,
 *     its index, the other worlds, or which of the optional arrays were asked for.
 *   Calls.  Synchronous, on the handle's stream.  They read the current rows and write nothing of the state: stepping with
 *     encounter calls in between gives the bits of stepping alone.  Two launches whatever the number of worlds or their sizes:
 *     one over (world, tile of 256 targets) that evaluates the pairs — the same number of pairs as a step, without a division —
 *     and one small reduce with a block per world.  No floating-point atomics; nothing is read back before the end.  The device
 *     scratch belongs to the handle, is grown on demand and is freed with its other arrays.  out: host memory, one per world.
 *   nbody_encounters_of_f32 / _of_f64.  Pure host code, no device, no handle: one segment by the contract above — the CPU
 *     statement of it, the same bits.  self != 0: source j is target j itself (the bodies' case; the two arrays may be the same).
 *     They refuse negative counts, out NULL, a NULL array with a non-zero count, self != 0 with n_targets != n_sources, and
 *     n_sources > 2^31 - 1, with NBODY_ERR_INVALID and no message.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or launched, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "encounters": nothing uploaded; out NULL; unknown
 *     flag bits; NBODY_ENCOUNTERS_TRACERS on one of the four handles that have no tracer calls.  A NULL handle gives
 *     NBODY_ERR_INVALID without a message.
 *   Not offered: tracer-tracer pairs; the k nearest for k > 1; a device-pointer variant; anything for nbody_ctx contexts.
 *     (The minimum over the steps of a call: nbody_watch_* below.) */
typedef struct nbody_world_encounters { /* 12 fields of 8 bytes, no padding: 96 bytes */
  int64_t rows;          /* targets of the segment: the world's bodies, or its tracers */
  int64_t sources;       /* the world's bodies */
  int64_t live_pairs;    /* ordered (target, source) pairs the law evaluates */
  int64_t skipped_pairs; /* ordered pairs it drops (for bodies, j == i is not a pair and is not counted) */
  int64_t close_pairs;   /* live pairs with d2 < limit2 */
  int64_t close_rows;    /* targets with at least one close pair */
  int64_t isolated_rows; /* targets with no live pair (nn_index == -1) */
  int64_t min_row, min_source; /* the closest live pair; -1, -1 where the world has none */
  double min_d2;         /* its d2, widened; +inf where there is none */
  int64_t max_nn_row;    /* the target whose nearest neighbour is farthest; -1 where none */
  double max_nn_d2;      /* its nn_d2, widened; +0.0 where there is none */
} nbody_world_encounters;
#define NBODY_ENCOUNTERS_TRACERS 1u /* targets are the world's tracers, sources its bodies */
int nbody_encounters_ensemble(nbody_ensemble* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                              nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                              float* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_ensemble64(nbody_ensemble64* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                                nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                                double* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_ragged(nbody_ragged* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                            nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                            float* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_ragged64(nbody_ragged64* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                              nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                              double* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_restricted(nbody_restricted* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                                nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                                float* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_restricted64(nbody_restricted64* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                                  nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                                  double* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_rr(nbody_rr* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                        nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                        float* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_rr64(nbody_rr64* e, uint32_t flags, const float* limit2 /*[n_worlds] or NULL: params.clamp*/,
                          nbody_world_encounters* out /*[n_worlds]*/, int32_t* nn_index /*[rows] or NULL*/,
                          double* nn_d2 /*[rows] or NULL*/, uint32_t* close /*[rows] or NULL*/);
int nbody_encounters_of_f32(int64_t n_targets, const float* target_xy, int64_t n_sources, const float* source_xy, int self,
                            float limit2, nbody_world_encounters* out, int32_t* nn_index /*[n_targets] or NULL*/,
                            float* nn_d2 /*[n_targets] or NULL*/, uint32_t* close /*[n_targets] or NULL*/);
int nbody_encounters_of_f64(int64_t n_targets, const double* target_xy, int64_t n_sources, const double* source_xy, int self,
                            double limit2, nbody_world_encounters* out, int32_t* nn_index /*[n_targets] or NULL*/,
                            double* nn_d2 /*[n_targets] or NULL*/, uint32_t* close /*[n_targets] or NULL*/);

/* ---- a watched run of an ensemble: closest approach, close samples and escape step per target over the steps of a call ----
 * What a study asks of a run as a whole, for all eight handles above: how close did each tracer get to a body and at which
 * step, was it captured, when did it leave the frame, did the clamp ever decide a pair.  nbody_encounters_* and nbody_summary_*
 * answer for the current rows; a loop of update(delta, 1), encounters, download and a fold on the host answers for the run at
 * several times the run's own cost, with a host synchronisation per step.  A watch is the handle's *_update(delta, n_steps)
 * with the device sampling every world before, between and after its steps and folding the samples on the device.
 *   The prefix.  nbody_watch_<handle>: a closed set of eight, under a prefix of its own.
 *   Samples.  Sample s, 0 <= s <= n_steps, is the state after s steps of this call: the rows an nbody_encounters_* call at that
 *     point would read (the bodies' current positions, or the tracers').  Sample s is taken when s % stride == 0 (stride >= 1);
 *     with NBODY_WATCH_RESUME s = 0 is left out, so that a call that continues an earlier one does not look at the boundary
 *     state twice.  n_steps == 0 is allowed: one sample and no step, or with NBODY_WATCH_RESUME no sample at all.  Sample
 *     numbers in the outputs are these s — step counts relative to the call — not an index among the taken samples.
 *   Targets and sources.  As nbody_encounters_* states them: the targets are one world's bodies or, with NBODY_WATCH_TRACERS,
 *     one world's tracers; the sources are that world's bodies; a body's own row is not a pair.
 *   Per sample, per target.  (nn_d2, nn_index) of the encounters' contract and nothing else of it, in the same arithmetic word
 *     for word: the handle's precision T, dx = xj - xi, dy = yj - yi, sum = |dx| + |dy|, d2 = dx*dx + dy*dy, each one IEEE
 *     operation, nothing fused; a pair is live iff `sum` is a normal number; the lowest source index stands on a tie; the first
 *     live pair stands even at d2 = +inf.  Derived from them: the target HAS A CLOSE PAIR at s iff nn_index >= 0 and nn_d2 <
 *     limit2[k] (widened to double on the f64 handles; limit2 == NULL: params.clamp in every world; a NaN or zero limit is
 *     never close) — the targets with close > 0 in the encounters' report, because a live d2 is never NaN and some pair is
 *     below the limit exactly when the smallest is.  The target IS OUT at s iff its own position fails within_bounds
 *     (main.rs:224-226) under `height`: x, y in [0, height); a NaN position is out, and height == 0 makes every row out at the
 *     first sample.
 *   Per target over the call.  Arrays of nbody_watch_rows_f32 / _f64, host memory, one entry per target of all worlds, laid
 *     out as the handle's *_download (for the tracers: *_tracers_download) lays out that segment's rows; `rows` may be NULL
 *     (records only) and so may each of its arrays.
 *       min_d2, min_index, min_sample: the sample's (nn_d2, nn_index) with the smallest nn_d2 over the samples at which the
 *         target had a live pair, and that sample.  A later sample replaces the record on a strict `<` only: the earliest
 *         sample stands.  The first sample with a live pair stands even at +inf.  A target that never had one: +inf, -1,
 *         NBODY_WATCH_NEVER.
 *       first_close: the first sample with a close pair, or NBODY_WATCH_NEVER.  close_samples: how many samples had one.
 *       first_out: the first sample at which the target was out, or NBODY_WATCH_NEVER (a target that comes back keeps it).
 *   Per world.  One nbody_world_watch.  samples is the number of samples the call took (a function of n_steps, stride and the
 *     flags alone, the same in every world, whatever its rows).  min_* is the world's closest approach in the call: the
 *     smallest min_d2 over its targets that had a live pair; on a tie the earliest sample stands, then the lowest row;
 *     min_source is that row's min_index, min_d2 the T value widened (exact).  close_rows: targets with any close sample;
 *     close_row_samples: the sum of close_samples; first_close_sample, first_out_sample: the smallest over the targets;
 *     out_rows: targets that were out at some sample; isolated_rows: targets that never had a live pair (with samples == 0:
 *     all of them).
 *   Order-free.  Every output is an integer count or an extreme under a total order with the tie rules above — (d2, sample,
 *     row), and the lowest source index within a sample — so the contract is bit for bit, without a tolerance, and the kernels
 *     are free to cut the sources into chunks and to join in any shape.
 *   Independence.  A world's record and rows are a function of its own rows, delta, limit2[k], height, stride, n_steps and the
 *     flags alone: not of the number of worlds, its index, the other worlds, which of the optional arrays were asked for, or
 *     the launch it falls in on a ragged handle.
 *   The run is untouched.  After a watch the handle's rows — bodies and tracers, under EXACT, FAST and AUTO — are bit for bit
 *     those after *_update(delta, n_steps); its step count has advanced by n_steps and its delta-stream sequences are as after
 *     that update.
 *   Split over calls.  watch(n1) followed by watch(n2) with NBODY_WATCH_RESUME, n1 % stride == 0, merged as follows with
 *     the second call's sample numbers shifted by n1 (NBODY_WATCH_NEVER and -1 stay), is watch(n1 + n2) bit for bit.  Per
 *     target: the second call's (min_d2, min_index, min_sample) replaces the first's iff the second has min_index >= 0 and
 *     the first has min_index < 0 or the second's min_d2 is strictly smaller; first_close and first_out are the first call's
 *     unless it has NBODY_WATCH_NEVER; close_samples add.  Per world: rows and sources stay, samples, close_row_samples add;
 *     min_* is recomputed from the merged rows under (d2, sample, row), close_rows, out_rows and isolated_rows are counted
 *     over them, the two first_*_sample are their minima.  (The records alone do not merge: close_rows is a count of a union.)
 *   Calls.  Synchronous, on the handle's stream.  One sampling launch per taken sample, whatever the number of worlds or their
 *     sizes — the encounters' pair launch with a leaner pair — between the handle's own step launches (1, 2, at most
 *     NBODY_RAGGED_MAX_LAUNCHES or at most NBODY_RR_MAX_LAUNCHES per step), and one reduce launch at the end that makes the
 *     records.  Nothing is read back and there is no host synchronisation before the end of the call; no floating-point
 *     atomics; the first taken sample writes the running rows, so no pass clears them and stale scratch is never read.  The
 *     device scratch belongs to the handle, is grown on demand and is freed with its other arrays.  The call's seconds are
 *     booked under sum_gravity, as an update's are (`counter` may be NULL).  out: host memory, one record per world.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or enqueued, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "watch": nothing uploaded; out NULL; unknown flag
 *     bits; NBODY_WATCH_TRACERS on one of the four handles that have no tracer calls; n_steps < 0; stride < 1; height > 2^24.
 *     A NULL handle gives NBODY_ERR_INVALID without a message.  NBODY_WATCH_TRACERS on a restricted handle that holds no
 *     tracers, or for a world of an nbody_rr handle without them, gives rows == 0 records: zero counts, -1 indices and sample
 *     numbers, min_d2 = +inf (the steps are taken all the same).
 *   Not offered: tracer-tracer pairs; the k nearest for k > 1; a per-sample history; a device-pointer variant; anything for
 *     nbody_ctx contexts.  (A delta, a clamp, a number of steps and a stride per world: nbody_wsweep_* below.) */
typedef struct nbody_world_watch { /* 13 fields of 8 bytes, no padding: 104 bytes */
  int64_t rows;               /* targets of the segment: the world's bodies, or its tracers */
  int64_t sources;            /* the world's bodies */
  int64_t samples;            /* samples the call took */
  int64_t min_row, min_source, min_sample; /* the closest approach of the call; -1, -1, -1 where the world has none */
  double min_d2;              /* its d2, widened; +inf where there is none */
  int64_t close_rows;         /* targets with a close pair at some sample */
  int64_t close_row_samples;  /* (target, sample) combinations with a close pair */
  int64_t first_close_sample; /* the first sample at which some target had a close pair; -1 where none */
  int64_t out_rows;           /* targets that were out at some sample */
  int64_t first_out_sample;   /* the first sample at which some target was out; -1 where none */
  int64_t isolated_rows;      /* targets that never had a live pair */
} nbody_world_watch;
#define NBODY_WATCH_TRACERS 1u         /* targets are the world's tracers, sources its bodies */
#define NBODY_WATCH_RESUME 2u          /* the call continues an earlier one: sample 0 is left out */
#define NBODY_WATCH_NEVER 0xffffffffu  /* a sample number that did not occur */
typedef struct nbody_watch_rows_f32 { /* per target of all worlds; each may be NULL */
  float* min_d2;
  int32_t* min_index;
  uint32_t *min_sample, *first_close, *close_samples, *first_out;
} nbody_watch_rows_f32;
typedef struct nbody_watch_rows_f64 {
  double* min_d2;
  int32_t* min_index;
  uint32_t *min_sample, *first_close, *close_samples, *first_out;
} nbody_watch_rows_f64;
int nbody_watch_ensemble(nbody_ensemble* e, uint32_t flags, float delta, int n_steps, int stride,
                         const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                         nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                         nbody_counting* counter);
int nbody_watch_ensemble64(nbody_ensemble64* e, uint32_t flags, double delta, int n_steps, int stride,
                           const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                           nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                           nbody_counting* counter);
int nbody_watch_ragged(nbody_ragged* e, uint32_t flags, float delta, int n_steps, int stride,
                       const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                       nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                       nbody_counting* counter);
int nbody_watch_ragged64(nbody_ragged64* e, uint32_t flags, double delta, int n_steps, int stride,
                         const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                         nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                         nbody_counting* counter);
int nbody_watch_restricted(nbody_restricted* e, uint32_t flags, float delta, int n_steps, int stride,
                           const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                           nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                           nbody_counting* counter);
int nbody_watch_restricted64(nbody_restricted64* e, uint32_t flags, double delta, int n_steps, int stride,
                             const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                             nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                             nbody_counting* counter);
int nbody_watch_rr(nbody_rr* e, uint32_t flags, float delta, int n_steps, int stride,
                   const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                   nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                   nbody_counting* counter);
int nbody_watch_rr64(nbody_rr64* e, uint32_t flags, double delta, int n_steps, int stride,
                     const float* limit2 /*[n_worlds] or NULL: params.clamp*/, uint32_t height,
                     nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                     nbody_counting* counter);

/* ---- a watched sweep of an ensemble: a watched run in which every world has its own time step, clamp, steps and stride ----
 * The two halves of a parameter study in one call, for all eight handles above.  nbody_sweep_* gives every world a delta, a
 * clamp and a number of steps; nbody_watch_* asks a run as a whole how close each target got, whether the clamp decided a pair
 * and when a target left the frame — but steps every world by one delta under one params.clamp.  A watched sweep is the
 * handle's nbody_sweep_<handle>(delta, clamp, steps, n_steps) with the device sampling world k on world k's own schedule: a
 * softening sweep learns per world which targets that world's own clamp altered, and a convergence study with steps[k] = T /
 * delta[k] and stride[k] proportional to steps[k] samples every world at the same physical times.
 *   The prefix.  nbody_wsweep_<handle>, and nbody_wsweep_plan: the names under nbody_watch_, under nbody_sweep_ and under
 *     each handle's own prefix are closed sets, so these nine have a prefix of their own.
 *   Arguments.  delta, clamp, steps and n_steps as nbody_sweep_* takes them; stride and limit2 are host arrays of n_worlds
 *     elements as well, read during the call only.  stride == NULL: 1 in every world.  The flags are NBODY_WATCH_TRACERS and
 *     NBODY_WATCH_RESUME; out, rows, nbody_world_watch, nbody_watch_rows_f32 / _f64 and NBODY_WATCH_NEVER are the watch's.
 *   Run.  After the call the handle's rows — bodies and tracers, under EXACT, FAST and AUTO — are bit for bit those after
 *     nbody_sweep_<handle>(delta, clamp, steps, n_steps); its step count has advanced by n_steps and its delta-stream sequences
 *     are as after that sweep.
 *   Samples.  Sample s, 0 <= s <= n_steps, is the state after s steps of this call.  World k takes it iff s <= steps[k]
 *     (steps == NULL: n_steps), s % stride[k] == 0, and not (s == 0 with NBODY_WATCH_RESUME).  A world that has taken its
 *     steps stands still and is not sampled again.  Sample numbers in the outputs are these s, step counts of the call, as in
 *     a watch.
 *   Record.  samples is the world's own number of samples: steps[k] / stride[k] + 1, minus 1 with NBODY_WATCH_RESUME.
 *   Close.  limit2 == NULL: world k's limit is clamp[k]; with clamp == NULL as well, params.clamp.  A softening sweep then
 *     reports, per world, the targets whose force that world's own clamp altered.
 *   Per-world contract (all of it).  World k's record and its slice of every rows array are bit for bit what a handle of the
 *     same kind gives when it holds world k alone with params.clamp = clamp[k] and calls nbody_watch_<handle>(flags, delta[k],
 *     steps[k], stride[k], limit2 ? &limit2[k] : NULL, height, ...).  So every rule of the watch carries over world by world:
 *     the arithmetic, live pairs, the tie rules, order-freedom, and tracers against their own world's bodies.
 *   No samples.  A world takes none under NBODY_WATCH_RESUME with stride[k] > steps[k] (steps[k] == 0 among them), and so
 *     does every world when n_steps == 0 under NBODY_WATCH_RESUME.  Its record is the watch's no-sample record: samples 0,
 *     isolated_rows == rows, -1 indices and sample numbers, min_d2 = +inf.  Its rows are +inf, -1, NBODY_WATCH_NEVER,
 *     NBODY_WATCH_NEVER, 0, NBODY_WATCH_NEVER: written by the reduce, never stale scratch.
 *   Independence.  As the sweep and the watch state it, and: a world's record and rows do not depend on the other worlds'
 *     stride, nor on which sampling launches the other worlds caused.
 *   Split over calls.  wsweep(n1, steps1) followed by wsweep(n2, steps2) with NBODY_WATCH_RESUME, merged as the watch's split
 *     merges with the second call's sample numbers shifted by n1, is wsweep(n1 + n2, steps) bit for bit, where every world is
 *     of one of two kinds: it ran through the first call — steps1[k] == n1, n1 % stride[k] == 0, steps[k] = n1 + steps2[k] — or
 *     it was finished within it — steps2[k] == 0, steps[k] = steps1[k].
 *   Calls.  Synchronous, on the handle's stream.  The step launches of a sweep (1, 2, at most NBODY_RAGGED_MAX_LAUNCHES or at
 *     most NBODY_RR_MAX_LAUNCHES per step); one sampling launch for every s at which at least one world takes a sample and
 *     none for an s nobody samples — the blocks of a world that does not sample at s return before they stage anything; one
 *     reduce launch at the end.  Nothing is read back and there is no host synchronisation before the end of the call; no
 *     floating-point atomics.  A world's first taken sample writes its running rows and later ones fold into them, so no pass
 *     clears them.  The host finds the s that need a launch in time O(n_worlds + n_steps * distinct strides), not O(samples).
 *     The seconds are booked under sum_gravity (`counter` may be NULL).  The device scratch is the watch's and the sweep's,
 *     with one 16-byte schedule entry per world beside it, freed with the handle's other arrays.
 *   nbody_wsweep_plan.  Pure host code, no device, no handle: samples_of_world[k] is the record's samples of world k, and
 *     n_sampling_launches the number of s in [0, n_steps] at which some world samples; either may be NULL.  It refuses what
 *     the call refuses of these arguments — n_worlds < 1, n_steps < 0, a steps[k] outside [0, n_steps], a stride[k] < 1,
 *     unknown flag bits — with NBODY_ERR_INVALID and no message, and then writes nothing.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or enqueued, the message beginning with the handle's word
 *     ("ensemble", "ragged", "restricted", "ragged restricted") and naming "wsweep": the sweep's and the watch's together —
 *     nothing uploaded; out NULL; delta NULL; unknown flag bits; n_steps < 0; a steps[k] outside [0, n_steps] (the message
 *     names the world); NBODY_WATCH_TRACERS on one of the four handles that have no tracer calls; height > 2^24 — and a
 *     stride[k] < 1 (the message names the world).  n_steps == 0 is allowed: every world takes sample 0 alone, or nothing with
 *     NBODY_WATCH_RESUME.  A NULL handle gives NBODY_ERR_INVALID without a message.
 *   Not offered: a per-world height; a per-world arith; a per-sample history; a device-pointer variant; anything for
 *     nbody_ctx contexts. */
int nbody_wsweep_ensemble(nbody_ensemble* e, uint32_t flags, const float* delta, const float* clamp,
                          const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                          const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                          nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                          nbody_counting* counter);
int nbody_wsweep_ensemble64(nbody_ensemble64* e, uint32_t flags, const double* delta, const float* clamp,
                            const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                            const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                            nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                            nbody_counting* counter);
int nbody_wsweep_ragged(nbody_ragged* e, uint32_t flags, const float* delta, const float* clamp,
                        const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                        const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                        nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                        nbody_counting* counter);
int nbody_wsweep_ragged64(nbody_ragged64* e, uint32_t flags, const double* delta, const float* clamp,
                          const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                          const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                          nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                          nbody_counting* counter);
int nbody_wsweep_restricted(nbody_restricted* e, uint32_t flags, const float* delta, const float* clamp,
                            const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                            const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                            nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                            nbody_counting* counter);
int nbody_wsweep_restricted64(nbody_restricted64* e, uint32_t flags, const double* delta, const float* clamp,
                              const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                              const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                              nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                              nbody_counting* counter);
int nbody_wsweep_rr(nbody_rr* e, uint32_t flags, const float* delta, const float* clamp,
                    const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                    const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                    nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f32* rows /*NULL: records only*/,
                    nbody_counting* counter);
int nbody_wsweep_rr64(nbody_rr64* e, uint32_t flags, const double* delta, const float* clamp,
                      const int32_t* steps, int n_steps, const int32_t* stride /*[n_worlds] or NULL: 1*/,
                      const float* limit2 /*[n_worlds] or NULL: world k's own clamp*/, uint32_t height,
                      nbody_world_watch* out /*[n_worlds]*/, const nbody_watch_rows_f64* rows /*NULL: records only*/,
                      nbody_counting* counter);
int nbody_wsweep_plan(int64_t n_worlds, const int32_t* steps /*[n_worlds] or NULL: n_steps*/, int n_steps,
                      const int32_t* stride /*[n_worlds] or NULL: 1*/, uint32_t flags,
                      int64_t* samples_of_world /*[n_worlds] or NULL*/, int64_t* n_sampling_launches /*or NULL*/);

/* ---- resident runs: small worlds take a call's steps in one launch ----
 * Every stepping call above pays one launch per step.  A world of at most NBODY_RESIDENT_MAX_BODIES bodies is one block of
 * that launch in both precisions, the block stages the world whole in LDS and reads nothing another block writes — and yet
 * every step ends with a write to global memory and a launch boundary, and the next one stages the same rows again.  For a
 * seed ensemble of three-body scatterings or a time-step convergence study of a few dozen bodies run for 10^4 .. 10^6 steps
 * that round trip costs more than the step.  A resident run is nbody_sweep_<handle> through another route: one block per world
 * stages its world once, takes the world's steps of the call in a loop with positions and velocities in LDS, and writes the
 * rows back once.  The arithmetic of a step is the text the stepping kernels run.
 *   The prefix.  nbody_resident_<handle> for the four handles without tracers, and nbody_resident_plan: a closed set of five,
 *     under a prefix of its own.
 *   Arguments.  nbody_sweep_<handle>'s, word for word: delta [n_worlds] in the handle's precision, required; clamp [n_worlds]
 *     or NULL (params.clamp in every world); steps [n_worlds] with 0 <= steps[k] <= n_steps, or NULL (every world takes
 *     n_steps).  The call is stateless: nothing of it stays in the handle.
 *   Contract.  After the call every bit of the handle's positions and velocities is what it would be after
 *     nbody_sweep_<handle> with the same arguments, under EXACT, FAST and AUTO; the handle's step count has advanced by n_steps
 *     and its delta-stream sequences are as after that sweep.  So the sweep's promises hold world by world: EXACT is
 *     bit-identical to the oracle's update_direct of that world with its own delta, clamp and number of steps; FAST and AUTO are
 *     bit-identical to that world alone; the route is taken per world from its clamp; the AUTO decision per world and per step
 *     from the positions at the start of that step; a world that has taken its steps keeps its bits, whatever they are (-0.0,
 *     NaN payloads, infinities); a world's bits depend on no other world, and not on where the call is cut into launches.
 *   Launches.  One block of 256 threads per world.  A launch takes at most NBODY_RESIDENT_STEPS_PER_LAUNCH steps of the call,
 *     so that no single kernel runs long on a shared device: a call whose largest steps[k] is S enqueues
 *     ceil(S / NBODY_RESIDENT_STEPS_PER_LAUNCH) launches, none with S == 0.  Between launches the rows are in global memory at
 *     full precision, so the cut is invisible.  The kernels write the rows in place (a block owns its world's rows for the
 *     whole launch).  No host synchronisation before the end of the call, nothing read back, no device scratch beyond the
 *     sweep's table and, on a ragged handle, 8 bytes per world (its first row and size), freed with the rows.  The seconds are
 *     booked under sum_gravity (`counter` may be NULL).
 *   nbody_resident_plan.  Pure host code, no device, no handle: n_launches as above and lds_bytes, the dynamic LDS of a
 *     launch, which is that of the largest world — the stepping kernels' layout plus the velocities: 24 bytes per couple of
 *     bodies + 8 n in f32, 20 bytes per body of the size padded to 8 + 16 n in f64.  Either output may be NULL.
 *   Refusals.  NBODY_ERR_INVALID before anything is allocated or enqueued, the message beginning with the handle's word
 *     ("ensemble", "ragged") and naming "resident": nothing uploaded; delta NULL; n_steps < 0; a steps[k] outside [0, n_steps]
 *     (the message names the world); a world of more than NBODY_RESIDENT_MAX_BODIES bodies (on a ragged handle the message
 *     names the first such world; the whole call is refused and nothing moves).  n_steps == 0 after the checks is a no-op.  A
 *     NULL handle gives NBODY_ERR_INVALID without a message.  nbody_resident_plan refuses the same arguments, and n_worlds < 1
 *     or n_bodies NULL, with NBODY_ERR_INVALID and no message, and then writes nothing.
 *   Measured (profiles/ensemble_resident.txt: end-to-end call times on an MI355X, 1024 steps, against *_update of the same
 *     handle).  4096 worlds x 3 bodies: 1.9 ms against 6.0 ms in f32 EXACT, 3.7 against 7.0 ms in f64 FAST; 4096 x 64: 20.5
 *     against 22.5 ms in f32 EXACT, 5.9 against 8.9 ms in f32 FAST; 1024 x 256: 59.8 against 63.4 ms in f32 EXACT, 90.3 against
 *     93.1 ms in f64 EXACT, which is the longest full launch recorded.  The gain is the launches and the round trip through
 *     global memory, so it shrinks as the pairs per step grow: 3.2 x at 3 bodies, 1.03 .. 1.15 x at 256.  A resident run was
 *     slower than *_update at no recorded shape (the four above and a ragged handle of 1024 worlds of 3 .. 256 bodies, in f32
 *     and f64, under EXACT and FAST).
 *   Not offered: worlds above 256 bodies (several blocks of a world would have to meet once per step: nbody_sweep_* is the
 *     call); the four handles with tracers (a tracer block would have to carry its world's bodies forward itself); several tiny
 *     worlds packed into one block; a resident watch; anything for nbody_ctx contexts. */
#define NBODY_RESIDENT_MAX_BODIES 256          /* a world that is one block: tiles == 1 in both precisions */
#define NBODY_RESIDENT_STEPS_PER_LAUNCH 1024   /* a launch takes at most this many steps of the call */
int nbody_resident_ensemble  (nbody_ensemble*   e, const float*  delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter);
int nbody_resident_ensemble64(nbody_ensemble64* e, const double* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter);
int nbody_resident_ragged    (nbody_ragged*     e, const float*  delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter);
int nbody_resident_ragged64  (nbody_ragged64*   e, const double* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter);
int nbody_resident_plan(int64_t n_worlds, const int64_t* n_bodies /*[n_worlds]*/, const int32_t* steps /*[n_worlds] or NULL: n_steps*/,
                        int n_steps, int is_f64, int32_t* n_launches, int32_t* lds_bytes);

#endif /* NBODY_ENSEMBLE_H */
