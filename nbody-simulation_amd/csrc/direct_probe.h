// Launch interface of the direct sum at arbitrary points (direct_probe.hip; the driver is in direct_driver.hip, the C ABI
// nbody_accel_direct_at_f32 / _f64).  Internal to the library.
//
// The sources are the context's bodies in row order; the targets are caller points in a device array of their own, with no
// mass and no self term.  Every kernel here computes a target from its own position and the bodies alone: the summation
// order depends on the number of sources (the fixed source split of probe_gsplit_*), never on which or how many targets
// share the launch — so a target's bits do not change with the call it comes in (include/nbody_hip.h).
//
// f32 FAST is not here: it is the step's clamped packed pass (direct_kernels.hip, direct_fast<1, *, false, 2>), which reads its
// targets from DirectArgs::pos_all and its sources from DirectArgs::src_pos, launched with the two pointing at different arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nbody {

// Source splits (blockIdx.y) of the FAST passes, a function of the number of sources only.
int probe_gsplit_f32(int64_t n_src);  // a split of ~8192 sources: 4096 targets over 2^20 bodies still fill 256 CUs
int probe_gsplit_f64(int64_t n_src);  // a split of >= 4096 sources (65 536 bodies: the 16 splits of the f64 step)

// f32 EXACT: one ascending-row chain per target with the reference's operations (direct_exact with separate targets).
hipError_t launch_probe_exact_f32(hipStream_t s, const float2* src, const float* mass, int64_t n_src, const float2* tgt, int64_t n_tgt,
                                  float clamp, float2* acc);
// f32 FAST: the partial sums [gsplit][n_tgt] of the main pass added in ascending split order.
hipError_t launch_probe_finish_f32(hipStream_t s, const float2* partial, int gsplit, int64_t n_tgt, float2* acc);

// f64: EXACT one ascending chain per target (pair_term_select, as direct64_pass<false>); FAST the f64 FAST pair over
// probe_gsplit_f64(n_src) source splits, the partial sums [gsplit][n_tgt] added in split order.
hipError_t launch_probe_f64(hipStream_t s, const double2* src, const double* mass, int64_t n_src, const double2* tgt, int64_t n_tgt,
                            double clamp, bool fast, double2* partial, double2* acc);
// The FAST pass of launch_probe_f64 alone: partial[probe_gsplit_f64(n_src)][n_tgt], left for the caller to add in split order
// (the tracer step's finish integrates in the same kernel, tracers.h).
hipError_t launch_probe_fast_pass_f64(hipStream_t s, const double2* src, const double* mass, int64_t n_src, const double2* tgt, int64_t n_tgt,
                                      double clamp, double2* partial);
// flag |= 1 when a coordinate of xy lies outside the f64 FAST domain of direct64.h (the flag is not cleared here).
hipError_t launch_probe_domain_f64(hipStream_t s, const double* xy, int64_t n_doubles, int* flag);

}  // namespace nbody
