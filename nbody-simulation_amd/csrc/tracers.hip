// Tracers (tracers.h): the kernels that finish a direct step's tracers.  gfx950, wave64.
// Compiled with -ffp-contract=off: nothing fuses unless a kernel writes fma.
//
// One lane per tracer.  The FAST main passes are the probe call's (the step's clamped packed pass in f32, probe_pass_f64<true>
// in f64); what is here marks every tracer's route from its pre-step position, folds the partial sums, runs the EXACT chain (the
// arithmetic of probe_exact_f32 and probe_pass_f64<false, 8>, operation for operation) and integrates — each tracer once, by the
// kernel its mark names.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "direct_kernels.h"
#include "pair.h"
#include "tracers.h"

namespace nbody {
namespace {

constexpr int kTracerTile = 256;  // sources per LDS stage
constexpr int kTracerTB = 8;      // f64 EXACT: terms evaluated branch-free per block, then added in ascending j

// The step-level route: the word the bodies' step decided by (block-uniform).
__device__ __forceinline__ bool step_is_exact(const TracerRoute& r) {
  if (r.all_exact) return true;
  if (r.word_kind == kTracerWordState) return r.word[kFlagState] == 2;
  if (r.word_kind == kTracerWordDomain64) return r.word[0] != 0;
  return false;
}
// FAST's domain per coordinate: f32 as direct_hazard_scan (below 2^60, zero or at least 2^-22), f64 as direct64.h (below 2^100,
// zero or at least 2^-300); a NaN fails the first test.
__device__ __forceinline__ bool outside_fast(float v) {
  const float a = __builtin_fabsf(v);
  return !(a < kFastBig) || (a != 0.f && a < kFastTiny);
}
__device__ __forceinline__ bool outside_fast(double v) {
  const double a = __builtin_fabs(v);
  return !(a < 0x1p100) || (a != 0.0 && a < 0x1p-300);
}
template <class T2> __device__ __forceinline__ bool takes_exact(const TracerRoute& r, bool step_exact, T2 p) {
  return step_exact || (r.per_target && (outside_fast(p.x) || outside_fast(p.y)));
}

// The one decision per tracer and step, taken from the PRE-step position before anything is integrated: mark[t] = 1 the tracer takes
// EXACT (the fix-up pass), 0 it stays FAST (the finish).  Both finishing kernels read it, so a tracer that a step carries across the
// boundary of FAST's domain is still integrated once.  The first thread also leaves the tracers' own decision word in `state_out`
// (kFlagState: 1 the FAST main pass runs, 2 it returns at once), which gates the f32 main pass on the device.
template <class T2>
__global__ __launch_bounds__(256) void tracer_mark(const T2* __restrict__ pos, int64_t n, const TracerRoute r, uint8_t* __restrict__ mark,
                                                  int* __restrict__ state_out) {
  const bool step_exact = step_is_exact(r);
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) state_out[kFlagState] = step_exact ? 2 : 1;
  if (t < n) mark[t] = takes_exact(r, step_exact, pos[t]) ? 1 : 0;
}

// main.rs:419-423: v += a*dt; x += v*dt, multiply then add.
template <class T, class T2> __device__ __forceinline__ void integrate_tracer(T2* pos, T2* vel, int64_t t, T2 p, T ax, T ay, T dt) {
  T2 v = vel[t];
  v.x = v.x + ax * dt;
  v.y = v.y + ay * dt;
  const T vx = v.x * dt, vy = v.y * dt;
  vel[t] = v;
  pos[t] = T2{p.x + vx, p.y + vy};
}

// The tracers that stay FAST (not marked): the main pass's splits in ascending order (as probe_finish_f32 / probe_finish_f64),
// integrated.
template <class T, class T2>
__global__ __launch_bounds__(256) void tracer_finish(const T2* __restrict__ partial, int gsplit, int64_t n, T2* __restrict__ pos,
                                                    T2* __restrict__ vel, T dt, const uint8_t* __restrict__ mark) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n || mark[t]) return;
  const T2 p = pos[t];
  T ax, ay;
  if constexpr (sizeof(T) == 4) {
    ax = 0.f;
    ay = 0.f;
    for (int g = 0; g < gsplit; ++g) {
      const T2 q = partial[(int64_t)g * n + t];
      ax += q.x;
      ay += q.y;
    }
  } else {
    const T2 q0 = partial[t];
    ax = q0.x;
    ay = q0.y;
    for (int g = 1; g < gsplit; ++g) {
      const T2 q = partial[(int64_t)g * n + t];
      ax = ax + q.x;
      ay = ay + q.y;
    }
  }
  integrate_tracer<T, T2>(pos, vel, t, p, ax, ay, dt);
}

// The tracers that take EXACT (marked; all of them without marks): one ascending-row chain over every body, integrated.  The
// block's 256 lanes stage the sources 256 at a time in LDS; a lane that is not taking EXACT helps staging and evaluates nothing.
template <class T, class T2>
__global__ __launch_bounds__(256) void tracer_exact(const T2* __restrict__ src, const T* __restrict__ mass, int64_t n_src,
                                                   T2* __restrict__ pos, T2* __restrict__ vel, int64_t n, T clamp, T dt,
                                                   const uint8_t* __restrict__ mark) {
  __shared__ T2 s_pos[kTracerTile];
  __shared__ T s_m[kTracerTile];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n;
  const T2 p = live ? pos[t] : T2{(T)0, (T)0};
  const bool mine = live && (!mark || mark[t]);  // (no marks: EXACT for all, known to the host)
  if (!__syncthreads_or(mine ? 1 : 0)) return;
  T ax = (T)0, ay = (T)0;
  for (int64_t base = 0; base < n_src; base += kTracerTile) {
    __syncthreads();
    const int64_t j = base + threadIdx.x;
    if (j < n_src) {
      s_pos[threadIdx.x] = src[j];
      s_m[threadIdx.x] = mass[j];
    } else if constexpr (sizeof(T) == 8) {  // a short last stage: a NaN position is a skipped pair, a -0.0 term
      s_pos[threadIdx.x] = T2{(T)__builtin_nan(""), (T)__builtin_nan("")};
      s_m[threadIdx.x] = (T)0;
    }
    __syncthreads();
    if (!mine) continue;
    const int64_t left = n_src - base;
    if constexpr (sizeof(T) == 4) {
      const int cnt = left < kTracerTile ? (int)left : kTracerTile;
      int k = 0;
      for (; k + 4 <= cnt; k += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) pair_as_written<float>(p.x, p.y, s_pos[k + u].x, s_pos[k + u].y, s_m[k + u], clamp, ax, ay);
      }
      for (; k < cnt; ++k) pair_as_written<float>(p.x, p.y, s_pos[k].x, s_pos[k].y, s_m[k], clamp, ax, ay);
    } else {
      const int len = left < kTracerTile ? (int)((left + kTracerTB - 1) / kTracerTB * kTracerTB) : kTracerTile;
      for (int k0 = 0; k0 < len; k0 += kTracerTB) {
        double2 term[kTracerTB];
#pragma unroll
        for (int jj = 0; jj < kTracerTB; ++jj) {  // any order of evaluation ...
          const double2 q = s_pos[k0 + jj];
          term[jj] = pair_term_select(p.x, p.y, q.x, q.y, s_m[k0 + jj], clamp);
        }
#pragma unroll
        for (int jj = 0; jj < kTracerTB; ++jj) {  // ... one order of addition: ascending j
          ax = ax + term[jj].x;
          ay = ay + term[jj].y;
        }
      }
    }
  }
  if (mine) integrate_tracer<T, T2>(pos, vel, t, p, ax, ay, dt);
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

template <class T>
hipError_t launch_tracer_mark(hipStream_t s, const void* pos, int64_t n, const TracerRoute& r, uint8_t* mark, int* state_out) {
  using T2 = typename V2<T>::type;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((tracer_mark<T2>), dim3(blocks_of(n)), dim3(256), 0, s, (const T2*)pos, n, r, mark, state_out);
  return hipGetLastError();
}
template <class T>
hipError_t launch_tracer_finish(hipStream_t s, const void* partial, int gsplit, int64_t n, void* pos, void* vel, T delta, const uint8_t* mark) {
  using T2 = typename V2<T>::type;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((tracer_finish<T, T2>), dim3(blocks_of(n)), dim3(256), 0, s, (const T2*)partial, gsplit, n, (T2*)pos, (T2*)vel, delta, mark);
  return hipGetLastError();
}
template <class T>
hipError_t launch_tracer_exact(hipStream_t s, const void* src, const void* mass, int64_t n_src, void* pos, void* vel, int64_t n, T clamp,
                               T delta, const uint8_t* mark) {
  using T2 = typename V2<T>::type;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((tracer_exact<T, T2>), dim3(blocks_of(n)), dim3(256), 0, s, (const T2*)src, (const T*)mass, n_src, (T2*)pos, (T2*)vel, n,
                     clamp, delta, mark);
  return hipGetLastError();
}

template hipError_t launch_tracer_mark<float>(hipStream_t, const void*, int64_t, const TracerRoute&, uint8_t*, int*);
template hipError_t launch_tracer_mark<double>(hipStream_t, const void*, int64_t, const TracerRoute&, uint8_t*, int*);
template hipError_t launch_tracer_finish<float>(hipStream_t, const void*, int, int64_t, void*, void*, float, const uint8_t*);
template hipError_t launch_tracer_finish<double>(hipStream_t, const void*, int, int64_t, void*, void*, double, const uint8_t*);
template hipError_t launch_tracer_exact<float>(hipStream_t, const void*, const void*, int64_t, void*, void*, int64_t, float, float,
                                               const uint8_t*);
template hipError_t launch_tracer_exact<double>(hipStream_t, const void*, const void*, int64_t, void*, void*, int64_t, double, double,
                                                const uint8_t*);

}  // namespace nbody
