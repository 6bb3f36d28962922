// The direct sum at points that are not bodies (target_kernels.h): the kernels the step does not already have.  gfx950, wave64.
// Compiled with -ffp-contract=off: nothing fuses unless a kernel writes fma.
//
// One lane per target; a block's 256 lanes walk the same sources, staged 256 at a time in LDS (every lane reads the same
// address: a broadcast).  The targets come from their own array, so there is no self term: a target on a body meets that
// body's pair like any other, and the reference's is_normal skip drops it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "direct_kernels.h"
#include "fast_domain.h"
#include "pair.h"
#include "target_kernels.h"

namespace nbody {
namespace {

constexpr int kTile = 256;  // sources per LDS stage
constexpr int kTB = 8;      // f64: terms evaluated branch-free per block, then added in ascending j

// The EXACT chain over one LDS stage with `left` sources still to come, per precision.
// f32: src/main.rs:236-252 operation by operation (pair_as_written<float>, the arithmetic of direct_exact's exact_pair).
__device__ __forceinline__ void exact_stage(float2 p, const float2* s_pos, const float* s_m, int64_t left, float clamp, float& ax, float& ay) {
  const int cnt = left < kTile ? (int)left : kTile;
  int k = 0;
  for (; k + 4 <= cnt; k += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) pair_as_written<float>(p.x, p.y, s_pos[k + u].x, s_pos[k + u].y, s_m[k + u], clamp, ax, ay);
  }
  for (; k < cnt; ++k) pair_as_written<float>(p.x, p.y, s_pos[k].x, s_pos[k].y, s_m[k], clamp, ax, ay);
}
// f64: as direct64_pass<false, 8>.  A short last stage is padded to whole blocks with NaN positions (target_exact).
__device__ __forceinline__ void exact_stage(double2 p, const double2* s_pos, const double* s_m, int64_t left, double clamp, double& ax,
                                            double& ay) {
  const int len = left < kTile ? (int)((left + kTB - 1) / kTB * kTB) : kTile;
  for (int k0 = 0; k0 < len; k0 += kTB) {
    double2 term[kTB];
#pragma unroll
    for (int jj = 0; jj < kTB; ++jj) {  // any order of evaluation ...
      const double2 q = s_pos[k0 + jj];
      term[jj] = pair_term_select(p.x, p.y, q.x, q.y, s_m[k0 + jj], clamp);
    }
#pragma unroll
    for (int jj = 0; jj < kTB; ++jj) {  // ... one order of addition: ascending j
      ax = ax + term[jj].x;
      ay = ay + term[jj].y;
    }
  }
}

// EXACT: one sequential chain per target over every source in ascending row.  With marks (Out::kMarked) a lane whose target the
// policy does not take helps staging and evaluates nothing, and a block without any taker leaves at once.
template <class T, class Out>
__global__ __launch_bounds__(256) void target_exact(const typename V2<T>::type* __restrict__ src, const T* __restrict__ mass, int64_t n_src,
                                                   const typename V2<T>::type* tgt, int64_t n_tgt, T clamp, const Out out) {
  using T2 = typename V2<T>::type;
  __shared__ T2 s_pos[kTile];
  __shared__ T s_m[kTile];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n_tgt;
  const T2 p = live ? tgt[t] : T2{(T)0, (T)0};
  bool mine = live;
  if constexpr (Out::kMarked) {
    mine = live && out.takes(t);
    if (!__syncthreads_or(mine ? 1 : 0)) return;
  }
  T ax = (T)0, ay = (T)0;
  for (int64_t base = 0; base < n_src; base += kTile) {
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
    if constexpr (Out::kMarked) {
      if (!mine) continue;
    }
    exact_stage(p, s_pos, s_m, n_src - base, clamp, ax, ay);
  }
  if (mine) out(t, ax, ay);
}

// FAST: the main pass's splits in ascending order.  The two precisions start differently and that is visible in the bits: f32
// starts from zero (as direct_finish: 0 + split 0 turns a -0 sum into +0), f64 from split 0 itself (as direct64_finish).  The
// probe call and the tracers share this one text, so they cannot drift apart.
template <class T, class Out>
__global__ __launch_bounds__(256) void target_fold(const typename V2<T>::type* __restrict__ partial, int gsplit, int64_t n_tgt, const Out out) {
  using T2 = typename V2<T>::type;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tgt || !out.takes(t)) return;
  constexpr int first = sizeof(T) == 4 ? 0 : 1;
  T2 s = first == 0 ? T2{(T)0, (T)0} : partial[t];
  for (int g = first; g < gsplit; ++g) {
    const T2 r = partial[(int64_t)g * n_tgt + t];
    s.x = s.x + r.x;
    s.y = s.y + r.y;
  }
  out(t, s.x, s.y);
}

// f64 FAST main pass: direct64_pass<true> with the targets apart.  One source split (blockIdx.y) per launch row, its partial sum to
// partial[split][t]; a short last stage is padded with massless sources (+-0).
__global__ __launch_bounds__(256) void target_fast_pass_f64(const double2* __restrict__ src, const double* __restrict__ mass, int64_t n_src,
                                                           const double2* __restrict__ tgt, int64_t n_tgt, double clamp, int gsplit,
                                                           double2* __restrict__ out) {
  __shared__ double2 s_pos[kTile];
  __shared__ double s_m[kTile];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n_tgt;
  const double2 p = live ? tgt[t] : double2{0.0, 0.0};
  const int64_t per = ((n_src + gsplit - 1) / gsplit + kTile - 1) / kTile * kTile;
  int64_t src_begin = (int64_t)blockIdx.y * per;
  if (src_begin > n_src) src_begin = n_src;
  const int64_t src_end = src_begin + per < n_src ? src_begin + per : n_src;
  double ax = 0.0, ay = 0.0;
  for (int64_t base = src_begin; base < src_end; base += kTile) {
    __syncthreads();
    const int64_t j = base + threadIdx.x;
    if (j < src_end) {
      s_pos[threadIdx.x] = src[j];
      s_m[threadIdx.x] = mass[j];
    } else {
      s_pos[threadIdx.x] = double2{0.0, 0.0};
      s_m[threadIdx.x] = 0.0;
    }
    __syncthreads();
    const int64_t left = src_end - base;
    const int len = left < kTile ? (int)((left + kTB - 1) / kTB * kTB) : kTile;
    for (int k0 = 0; k0 < len; k0 += kTB) {
#pragma unroll
      for (int jj = 0; jj < kTB; ++jj) {
        const double2 q = s_pos[k0 + jj];
        pair_fast(p.x, p.y, q.x, q.y, s_m[k0 + jj], clamp, ax, ay);
      }
    }
  }
  if (live) out[(int64_t)blockIdx.y * n_tgt + t] = double2{ax, ay};
}

// The bodies' f64 FAST domain (direct64_domain_scan over an array of its own flag).
__global__ __launch_bounds__(256) void target_domain_scan_f64(const double* __restrict__ xy, int64_t n_doubles, int* flag) {
  bool out = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_doubles; i += (int64_t)gridDim.x * 256) out |= outside_fast(xy[i]);
  if (__builtin_amdgcn_ballot_w64(out) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// The step-level route: the word the bodies' step decided by (block-uniform).
__device__ __forceinline__ bool step_is_exact(const TracerRoute& r) {
  if (r.all_exact) return true;
  if (r.word_kind == kTracerWordState) return r.word[kFlagState] == 2;
  if (r.word_kind == kTracerWordDomain64) return r.word[0] != 0;
  return false;
}
// The one decision per tracer and step, taken from the PRE-step position before anything is integrated: mark[t] = 1 the tracer takes
// EXACT (the fix-up pass), 0 it stays FAST (the fold).  Both finishing kernels read it, so a tracer that a step carries across the
// boundary of FAST's domain is still integrated once.  The first thread also leaves the tracers' own decision word in `state_out`
// (kFlagState: 1 the FAST main pass runs, 2 it returns at once), which gates the f32 main pass on the device.
template <class T2>
__global__ __launch_bounds__(256) void tracer_mark(const T2* __restrict__ pos, int64_t n, const TracerRoute r, uint8_t* __restrict__ mark,
                                                  int* __restrict__ state_out) {
  const bool step_exact = step_is_exact(r);
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) state_out[kFlagState] = step_exact ? 2 : 1;
  if (t >= n) return;
  const T2 p = pos[t];
  mark[t] = step_exact || (r.per_target && (outside_fast(p.x) || outside_fast(p.y))) ? 1 : 0;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int probe_gsplit_f32(int64_t n_src) {
  const int64_t g = (n_src + 8191) / 8192;
  return (int)(g < 1 ? 1 : (g > 128 ? 128 : g));
}
int probe_gsplit_f64(int64_t n_src) {
  const int64_t g = (n_src + 4095) / 4096;
  return (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
}

template <class T, class Out>
hipError_t launch_target_exact(hipStream_t s, const typename V2<T>::type* src, const T* mass, int64_t n_src, const typename V2<T>::type* tgt,
                               int64_t n_tgt, T clamp, const Out& out) {
  if (n_tgt <= 0) return hipSuccess;
  hipLaunchKernelGGL((target_exact<T, Out>), dim3(blocks_of(n_tgt)), dim3(256), 0, s, src, mass, n_src, tgt, n_tgt, clamp, out);
  return hipGetLastError();
}
template <class T, class Out>
hipError_t launch_target_fold(hipStream_t s, const typename V2<T>::type* partial, int gsplit, int64_t n_tgt, const Out& out) {
  if (n_tgt <= 0) return hipSuccess;
  hipLaunchKernelGGL((target_fold<T, Out>), dim3(blocks_of(n_tgt)), dim3(256), 0, s, partial, gsplit, n_tgt, out);
  return hipGetLastError();
}
#define NB_TARGET_LAUNCHERS(T, Out)                                                                                                  \
  template hipError_t launch_target_exact<T, Out>(hipStream_t, const V2<T>::type*, const T*, int64_t, const V2<T>::type*, int64_t, T, \
                                                  const Out&);                                                                       \
  template hipError_t launch_target_fold<T, Out>(hipStream_t, const V2<T>::type*, int, int64_t, const Out&);
NB_TARGET_LAUNCHERS(float, StoreAcc<float>)
NB_TARGET_LAUNCHERS(float, StepTracer<float>)
NB_TARGET_LAUNCHERS(double, StoreAcc<double>)
NB_TARGET_LAUNCHERS(double, StepTracer<double>)
#undef NB_TARGET_LAUNCHERS

hipError_t launch_target_fast_pass_f64(hipStream_t s, const double2* src, const double* mass, int64_t n_src, const double2* tgt, int64_t n_tgt,
                                       double clamp, double2* partial) {
  if (n_tgt <= 0) return hipSuccess;
  const int g = probe_gsplit_f64(n_src);
  hipLaunchKernelGGL(target_fast_pass_f64, dim3(blocks_of(n_tgt), (unsigned)g), dim3(256), 0, s, src, mass, n_src, tgt, n_tgt, clamp, g, partial);
  return hipGetLastError();
}

hipError_t launch_domain_scan_f64(hipStream_t s, const double* xy, int64_t n_doubles, int* flag) {
  if (n_doubles <= 0) return hipSuccess;
  int64_t blocks = (n_doubles + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(target_domain_scan_f64, dim3((unsigned)blocks), dim3(256), 0, s, xy, n_doubles, flag);
  return hipGetLastError();
}

template <class T>
hipError_t launch_tracer_mark(hipStream_t s, const typename V2<T>::type* pos, int64_t n, const TracerRoute& r, uint8_t* mark, int* state_out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((tracer_mark<typename V2<T>::type>), dim3(blocks_of(n)), dim3(256), 0, s, pos, n, r, mark, state_out);
  return hipGetLastError();
}
template hipError_t launch_tracer_mark<float>(hipStream_t, const float2*, int64_t, const TracerRoute&, uint8_t*, int*);
template hipError_t launch_tracer_mark<double>(hipStream_t, const double2*, int64_t, const TracerRoute&, uint8_t*, int*);

}  // namespace nbody
