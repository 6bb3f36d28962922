// The direct sum at arbitrary points (direct_probe.h): the kernels the step does not already have.  gfx950, wave64.
// Compiled with -ffp-contract=off: nothing fuses unless a kernel writes fma.
//
// One lane per target; a block's 256 lanes walk the same sources, staged 256 at a time in LDS (every lane reads the same
// address: a broadcast).  The targets come from their own array, so there is no self term: a target on a body meets that
// body's pair like any other, and the reference's is_normal skip drops it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "direct_probe.h"
#include "pair.h"

namespace nbody {
namespace {

constexpr int kProbeTile = 256;  // sources per LDS stage

// f32 EXACT: src/main.rs:236-252 operation by operation (pair_as_written<float>, the arithmetic of direct_exact's exact_pair),
// one sequential chain per target in ascending row.
__global__ __launch_bounds__(256) void probe_exact_f32(const float2* __restrict__ src, const float* __restrict__ mass, int64_t n_src,
                                                      const float2* __restrict__ tgt, int64_t n_tgt, float clamp, float2* __restrict__ acc) {
  __shared__ float2 s_pos[kProbeTile];
  __shared__ float s_m[kProbeTile];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n_tgt;
  const float2 p = live ? tgt[t] : make_float2(0.f, 0.f);
  float ax = 0.f, ay = 0.f;
  for (int64_t base = 0; base < n_src; base += kProbeTile) {
    __syncthreads();
    const int64_t j = base + threadIdx.x;
    if (j < n_src) {
      s_pos[threadIdx.x] = src[j];
      s_m[threadIdx.x] = mass[j];
    }
    __syncthreads();
    const int cnt = n_src - base < kProbeTile ? (int)(n_src - base) : kProbeTile;
    int k = 0;
    for (; k + 4 <= cnt; k += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) pair_as_written<float>(p.x, p.y, s_pos[k + u].x, s_pos[k + u].y, s_m[k + u], clamp, ax, ay);
    }
    for (; k < cnt; ++k) pair_as_written<float>(p.x, p.y, s_pos[k].x, s_pos[k].y, s_m[k], clamp, ax, ay);
  }
  if (live) acc[t] = make_float2(ax, ay);
}

// f32 FAST: the main pass's splits in ascending order (direct_finish without the near sources and the integration).
__global__ __launch_bounds__(256) void probe_finish_f32(const float2* __restrict__ partial, int gsplit, int64_t n_tgt,
                                                       float2* __restrict__ acc) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tgt) return;
  float ax = 0.f, ay = 0.f;
  for (int g = 0; g < gsplit; ++g) {
    const float2 r = partial[(int64_t)g * n_tgt + t];
    ax += r.x;
    ay += r.y;
  }
  acc[t] = make_float2(ax, ay);
}

// f64: direct64_pass with the targets apart from the sources.  FAST: one source split (blockIdx.y) per launch row, its partial
// sum to partial[split][t]; EXACT: one chain over every source, TB terms evaluated branch-free and then added in ascending j.
template <bool FAST, int TB>
__global__ __launch_bounds__(256) void probe_pass_f64(const double2* __restrict__ src, const double* __restrict__ mass, int64_t n_src,
                                                     const double2* __restrict__ tgt, int64_t n_tgt, double clamp, int gsplit,
                                                     double2* __restrict__ out) {
  static_assert(kProbeTile % TB == 0, "term blocks tile the LDS stage");
  __shared__ double2 s_pos[kProbeTile];
  __shared__ double s_m[kProbeTile];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n_tgt;
  const double2 p = live ? tgt[t] : double2{0.0, 0.0};
  int64_t src_begin = 0, src_end = n_src;
  if constexpr (FAST) {
    const int64_t per = ((n_src + gsplit - 1) / gsplit + kProbeTile - 1) / kProbeTile * kProbeTile;
    src_begin = (int64_t)blockIdx.y * per;
    if (src_begin > n_src) src_begin = n_src;
    src_end = src_begin + per < n_src ? src_begin + per : n_src;
  }
  // padding of a short last stage: EXACT a NaN position (the pair is skipped: a -0.0 term), FAST a massless source (+-0)
  const double pad = FAST ? 0.0 : __builtin_nan("");
  double ax = 0.0, ay = 0.0;
  for (int64_t base = src_begin; base < src_end; base += kProbeTile) {
    __syncthreads();
    const int64_t j = base + threadIdx.x;
    if (j < src_end) {
      s_pos[threadIdx.x] = src[j];
      s_m[threadIdx.x] = mass[j];
    } else {
      s_pos[threadIdx.x] = double2{pad, pad};
      s_m[threadIdx.x] = 0.0;
    }
    __syncthreads();
    const int64_t left = src_end - base;
    const int len = left < kProbeTile ? (int)((left + TB - 1) / TB * TB) : kProbeTile;
    for (int k0 = 0; k0 < len; k0 += TB) {
      if constexpr (FAST) {
#pragma unroll
        for (int jj = 0; jj < TB; ++jj) {
          const double2 q = s_pos[k0 + jj];
          pair_fast(p.x, p.y, q.x, q.y, s_m[k0 + jj], clamp, ax, ay);
        }
      } else {
        double2 term[TB];
#pragma unroll
        for (int jj = 0; jj < TB; ++jj) {  // any order of evaluation ...
          const double2 q = s_pos[k0 + jj];
          term[jj] = pair_term_select(p.x, p.y, q.x, q.y, s_m[k0 + jj], clamp);
        }
#pragma unroll
        for (int jj = 0; jj < TB; ++jj) {  // ... one order of addition: ascending j
          ax = ax + term[jj].x;
          ay = ay + term[jj].y;
        }
      }
    }
  }
  if (!live) return;
  out[(FAST ? (int64_t)blockIdx.y * n_tgt : 0) + t] = double2{ax, ay};
}

// probe_finish_f64 and probe_domain_f64 restate direct64_finish and direct64_domain_scan (direct64.hip) for the targets apart
// rather than share them, so that the f64 step's code object stays as it is: a change to the f64 FAST domain or to the order in
// which the splits are added belongs in both places.
__global__ __launch_bounds__(256) void probe_finish_f64(const double2* __restrict__ partial, int gsplit, int64_t n_tgt,
                                                       double2* __restrict__ acc) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tgt) return;
  double2 s = partial[t];
  for (int g = 1; g < gsplit; ++g) {
    const double2 r = partial[(int64_t)g * n_tgt + t];
    s.x = s.x + r.x;
    s.y = s.y + r.y;
  }
  acc[t] = s;
}

// The FAST domain of direct64.h: finite, below 2^100 in magnitude, zero or at least 2^-300.
__global__ __launch_bounds__(256) void probe_domain_f64(const double* __restrict__ xy, int64_t n_doubles, int* flag) {
  bool out = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_doubles; i += (int64_t)gridDim.x * 256) {
    const double v = __builtin_fabs(xy[i]);
    out |= !(v < 0x1p100) || (v != 0.0 && v < 0x1p-300);  // (a NaN fails the first test)
  }
  if (__builtin_amdgcn_ballot_w64(out) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

unsigned blocks_of(int64_t n_tgt) { return (unsigned)((n_tgt + 255) / 256); }

}  // namespace

int probe_gsplit_f32(int64_t n_src) {
  const int64_t g = (n_src + 8191) / 8192;
  return (int)(g < 1 ? 1 : (g > 128 ? 128 : g));
}
int probe_gsplit_f64(int64_t n_src) {
  const int64_t g = (n_src + 4095) / 4096;
  return (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
}

hipError_t launch_probe_exact_f32(hipStream_t s, const float2* src, const float* mass, int64_t n_src, const float2* tgt, int64_t n_tgt,
                                  float clamp, float2* acc) {
  if (n_tgt <= 0) return hipSuccess;
  hipLaunchKernelGGL(probe_exact_f32, dim3(blocks_of(n_tgt)), dim3(256), 0, s, src, mass, n_src, tgt, n_tgt, clamp, acc);
  return hipGetLastError();
}

hipError_t launch_probe_finish_f32(hipStream_t s, const float2* partial, int gsplit, int64_t n_tgt, float2* acc) {
  if (n_tgt <= 0) return hipSuccess;
  hipLaunchKernelGGL(probe_finish_f32, dim3(blocks_of(n_tgt)), dim3(256), 0, s, partial, gsplit, n_tgt, acc);
  return hipGetLastError();
}

hipError_t launch_probe_f64(hipStream_t s, const double2* src, const double* mass, int64_t n_src, const double2* tgt, int64_t n_tgt,
                            double clamp, bool fast, double2* partial, double2* acc) {
  if (n_tgt <= 0) return hipSuccess;
  if (!fast) {
    hipLaunchKernelGGL((probe_pass_f64<false, 8>), dim3(blocks_of(n_tgt)), dim3(256), 0, s, src, mass, n_src, tgt, n_tgt, clamp, 1, acc);
    return hipGetLastError();
  }
  hipError_t e = launch_probe_fast_pass_f64(s, src, mass, n_src, tgt, n_tgt, clamp, partial);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(probe_finish_f64, dim3(blocks_of(n_tgt)), dim3(256), 0, s, partial, probe_gsplit_f64(n_src), n_tgt, acc);
  return hipGetLastError();
}

hipError_t launch_probe_fast_pass_f64(hipStream_t s, const double2* src, const double* mass, int64_t n_src, const double2* tgt, int64_t n_tgt,
                                      double clamp, double2* partial) {
  if (n_tgt <= 0) return hipSuccess;
  const int g = probe_gsplit_f64(n_src);
  hipLaunchKernelGGL((probe_pass_f64<true, 8>), dim3(blocks_of(n_tgt), (unsigned)g), dim3(256), 0, s, src, mass, n_src, tgt, n_tgt, clamp, g,
                     partial);
  return hipGetLastError();
}

hipError_t launch_probe_domain_f64(hipStream_t s, const double* xy, int64_t n_doubles, int* flag) {
  if (n_doubles <= 0) return hipSuccess;
  int64_t blocks = (n_doubles + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(probe_domain_f64, dim3((unsigned)blocks), dim3(256), 0, s, xy, n_doubles, flag);
  return hipGetLastError();
}

}  // namespace nbody
