// Launch interface of the tracer kernels (tracers.hip; the drivers are in direct_driver.hip and tree_driver.hip, the C ABI
// nbody_tracers_*).  Internal to the library.
//
// Tracers are points without mass that step with the bodies: in every step a tracer takes the field of the bodies at their
// pre-step positions and integrates as main.rs:419-423 (v += a*dt; x += v*dt, multiply then add).  They live in device arrays
// of their own (ctx.h, Tracers) in upload order.  A tracer's bits depend on its own state and the bodies alone: the FAST main
// passes are the probe call's (direct_probe.h), whose summation order is fixed by the number of bodies, and every kernel here
// works lane by lane.
//
// A direct step routes its tracers on the device:
//   - the step-level route is the decision word the bodies' own step left in its workspace (f32 AUTO: kFlagState == 2, a body
//     outside FAST's domain; f64 FAST: the domain flag of direct64.hip) — `word`, read by the kernels, never by the host;
//   - under f32 AUTO and f64 FAST a tracer outside FAST's domain takes its EXACT value (`per_target`).
// launch_tracer_mark takes that decision ONCE per tracer and step, from the pre-step positions and before anything is integrated:
// mark[t] = 1 the tracer takes EXACT.  launch_tracer_finish completes the unmarked tracers (partial sums in split order, then the
// integration); launch_tracer_exact runs the EXACT chain for the marked ones and integrates them; a block with none of them leaves at
// once.  Both read the same marks, so every tracer is integrated by exactly one of the two wherever the step carries it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nbody {

enum { kTracerWordNone = 0, kTracerWordState = 1, kTracerWordDomain64 = 2 };
struct TracerRoute {
  const int* word = nullptr;  // the bodies' decision words (device), or null
  int word_kind = kTracerWordNone;
  int all_exact = 0;          // host-known: EXACT arithmetic, a clamp outside FAST's range, no bodies
  int per_target = 0;         // a tracer outside FAST's domain takes its EXACT value
};

// pos: all n tracers; mark: [n]; state_out: decision words of the tracers' own (direct_kernels.h) — kFlagState receives 1 when the
// FAST main pass is to run and 2 when the step-level route is EXACT (DirectArgs::flags / run_state = 1 gate the f32 pass with it).
template <class T> hipError_t launch_tracer_mark(hipStream_t s, const void* pos, int64_t n, const TracerRoute& r, uint8_t* mark, int* state_out);
// pos, vel, mark: the tracers [n] (a batch: `partial` is [gsplit][n]); T = float or double.
template <class T>
hipError_t launch_tracer_finish(hipStream_t s, const void* partial, int gsplit, int64_t n, void* pos, void* vel, T delta, const uint8_t* mark);
// src, mass: the bodies at their pre-step positions, in row order.  mark == nullptr: every tracer (EXACT known to the host).
template <class T>
hipError_t launch_tracer_exact(hipStream_t s, const void* src, const void* mass, int64_t n_src, void* pos, void* vel, int64_t n, T clamp,
                               T delta, const uint8_t* mark);

}  // namespace nbody
