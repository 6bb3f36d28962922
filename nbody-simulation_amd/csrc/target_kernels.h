// Launch interface of the direct sum at points that are not bodies (target_kernels.hip; the driver is target_driver.hip): the
// probe call (nbody_accel_direct_at_f32 / _f64) and the tracers' share of a direct step.  Internal to the library.
//
// The sources are the context's bodies in row order; the targets live in a device array of their own, with no mass and no self
// term.  Every kernel computes a target from its own position and the bodies alone: the summation order depends on the number of
// sources (the fixed source split of probe_gsplit_*), never on which or how many targets share the launch — so a target's bits do
// not change with the call it comes in (include/nbody_hip.h), and a tracer's FAST value is the probe call's.
//
// Both callers run the same two kernels, target_exact (one ascending-row chain per target) and target_fold (the FAST partial sums
// in split order), and differ in what becomes of the sum — the output policy: StoreAcc writes it, StepTracer integrates the tracer.
//
// f32 FAST's main pass is not here: it is the step's clamped packed pass (direct_kernels.hip, direct_fast<1, *, false, 2>), which
// reads its targets from DirectArgs::pos_all and its sources from DirectArgs::src_pos, launched with the two pointing at different
// arrays.
//
// A direct step routes its tracers on the device:
//   - the step-level route is the decision word the bodies' own step left in its workspace (f32 AUTO: kFlagState == 2, a body
//     outside FAST's domain; f64 FAST: the domain flag of direct64.hip) — `word`, read by the kernels, never by the host;
//   - under f32 AUTO and f64 FAST a tracer outside FAST's domain takes its EXACT value (`per_target`).
// launch_tracer_mark takes that decision ONCE per tracer and step, from the pre-step positions and before anything is integrated:
// mark[t] = 1 the tracer takes EXACT.  target_fold completes the unmarked tracers and target_exact the marked ones (a block with
// none of them leaves at once).  Both read the same marks, so every tracer is integrated by exactly one of the two wherever the
// step carries it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pair.h"

namespace nbody {

// ---- output policies: what target_exact and target_fold do with the sum of target t
// The probe call: the acceleration itself.
template <class T> struct StoreAcc {
  using T2 = typename V2<T>::type;
  static constexpr bool kMarked = false;
  T2* acc;
  __device__ bool takes(int64_t) const { return true; }
  __device__ void operator()(int64_t t, T ax, T ay) const { acc[t] = T2{ax, ay}; }
};
// A tracer: main.rs:419-423 (v += a*dt; x += v*dt, multiply then add), for the tracers whose mark equals `want` (mark == nullptr:
// every tracer — EXACT known to the host).
template <class T> struct StepTracer {
  using T2 = typename V2<T>::type;
  static constexpr bool kMarked = true;
  T2* pos;
  T2* vel;
  T dt;
  const uint8_t* mark;
  uint8_t want;
  __device__ bool takes(int64_t t) const { return !mark || mark[t] == want; }
  __device__ void operator()(int64_t t, T ax, T ay) const {
    T2 v = vel[t];
    const T2 p = pos[t];
    v.x = v.x + ax * dt;
    v.y = v.y + ay * dt;
    const T vx = v.x * dt, vy = v.y * dt;
    vel[t] = v;
    pos[t] = T2{p.x + vx, p.y + vy};
  }
};

// Source splits (blockIdx.y) of the FAST passes, a function of the number of sources only.
int probe_gsplit_f32(int64_t n_src);  // a split of ~8192 sources: 4096 targets over 2^20 bodies still fill 256 CUs
int probe_gsplit_f64(int64_t n_src);  // a split of >= 4096 sources (65 536 bodies: the 16 splits of the f64 step)

// EXACT: one ascending-row chain per target with the reference's operations (f32: direct_exact's, f64: direct64_pass<false>'s).
// Out = StoreAcc<T> or StepTracer<T>; tgt: the positions of the n_tgt targets (a tracer step: out.pos, read before it is written).
template <class T, class Out>
hipError_t launch_target_exact(hipStream_t s, const typename V2<T>::type* src, const T* mass, int64_t n_src, const typename V2<T>::type* tgt,
                               int64_t n_tgt, T clamp, const Out& out);
// FAST: the main pass's partial sums [gsplit][n_tgt] added in ascending split order.
template <class T, class Out> hipError_t launch_target_fold(hipStream_t s, const typename V2<T>::type* partial, int gsplit, int64_t n_tgt, const Out& out);
// f64 FAST main pass (the f64 FAST pair, direct64_pass<true> with the targets apart): partial[probe_gsplit_f64(n_src)][n_tgt].
hipError_t launch_target_fast_pass_f64(hipStream_t s, const double2* src, const double* mass, int64_t n_src, const double2* tgt, int64_t n_tgt,
                                       double clamp, double2* partial);
// flag |= 1 when a coordinate of xy lies outside the f64 FAST domain (fast_domain.h; the flag is not cleared here).
hipError_t launch_domain_scan_f64(hipStream_t s, const double* xy, int64_t n_doubles, int* flag);

enum { kTracerWordNone = 0, kTracerWordState = 1, kTracerWordDomain64 = 2 };
struct TracerRoute {
  const int* word = nullptr;  // the bodies' decision words (device), or null
  int word_kind = kTracerWordNone;
  int all_exact = 0;          // host-known: EXACT arithmetic, a clamp outside FAST's range, no bodies
  int per_target = 0;         // a tracer outside FAST's domain takes its EXACT value
};
// pos: all n tracers; mark: [n]; state_out: decision words of the tracers' own (direct_kernels.h) — kFlagState receives 1 when the
// FAST main pass is to run and 2 when the step-level route is EXACT (DirectArgs::flags / run_state = 1 gate the f32 pass with it).
template <class T>
hipError_t launch_tracer_mark(hipStream_t s, const typename V2<T>::type* pos, int64_t n, const TracerRoute& r, uint8_t* mark, int* state_out);

}  // namespace nbody
