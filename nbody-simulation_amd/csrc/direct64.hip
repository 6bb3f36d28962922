// The f64 direct O(N^2) step: EXACT (bit-identical to the oracle) and FAST (opt-in, 1e-12 of sum|term|).  gfx950, wave64.
// Compiled with -ffp-contract=off: nothing fuses unless a kernel writes fma.  Semantics and the FAST domain: direct64.h.
//
// One lane per target; the block's 256 lanes walk the same sources, staged 256 at a time in LDS (every lane reads the same
// address: a broadcast).  A block of TB sources' terms is evaluated first, branch-free (pair_term_select, pair.h), and then
// added in ascending j, so the TB pairs' division chains are independent and overlap — the EXACT kernel is bound by the two
// compiler-expanded f64 divisions per pair.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "direct64.h"
#include "env.h"
#include "fast_domain.h"
#include "pair.h"

namespace nbody {
namespace {

constexpr int kTile64 = 256;        // sources per LDS stage
constexpr size_t kFlag64Bytes = 256;

// main.rs:419-423 in double (v += a*dt; x += v*dt, multiply then add), or the acceleration itself.
__device__ __forceinline__ void direct64_out(const Direct64Args& a, int64_t t, double ax, double ay) {
  if (a.acc_out) a.acc_out[t] = double2{ax, ay};
  if (a.vel) {
    double2 v = a.vel[t];
    const double2 p = a.pos[t];
    v.x = v.x + ax * a.delta;
    v.y = v.y + ay * a.delta;
    const double vx = v.x * a.delta, vy = v.y * a.delta;
    a.vel[t] = v;
    a.pos_out[t] = double2{p.x + vx, p.y + vy};
  }
}

// FAST: one source split (blockIdx.y) per launch row; EXACT: gsplit is 1 and the one chain covers every source.
template <bool FAST, int TB>
__global__ __launch_bounds__(256) void direct64_pass(const Direct64Args a) {
  static_assert(kTile64 % TB == 0, "term blocks tile the LDS stage");
  __shared__ double2 s_pos[kTile64];
  __shared__ double s_m[kTile64];
  if (a.domain_flag) {  // block-uniform: FAST runs inside the domain, EXACT is then the fallback for the steps outside it
    const int out = *a.domain_flag;
    if (FAST ? out != 0 : out == 0) return;
  }
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < a.n;
  const double2 p = live ? a.pos[t] : double2{0.0, 0.0};
  const double clamp = a.clamp;
  int64_t src_begin = 0, src_end = a.n;
  if constexpr (FAST) {
    const int64_t per = ((a.n + a.gsplit - 1) / a.gsplit + kTile64 - 1) / kTile64 * kTile64;
    src_begin = (int64_t)blockIdx.y * per;
    src_end = src_begin + per < a.n ? src_begin + per : a.n;
  }
  // padding of a short last stage: EXACT a NaN position (the pair is skipped: a -0.0 term), FAST a massless source (+-0)
  const double pad = FAST ? 0.0 : __builtin_nan("");
  double ax = 0.0, ay = 0.0;
  for (int64_t base = src_begin; base < src_end; base += kTile64) {
    __syncthreads();
    const int64_t j = base + threadIdx.x;
    if (j < src_end) {
      s_pos[threadIdx.x] = a.pos[j];
      s_m[threadIdx.x] = a.mass[j];
    } else {
      s_pos[threadIdx.x] = double2{pad, pad};
      s_m[threadIdx.x] = 0.0;
    }
    __syncthreads();
    const int64_t left = src_end - base;
    const int len = left < kTile64 ? (int)((left + TB - 1) / TB * TB) : kTile64;
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
  if (FAST && a.gsplit > 1) {
    a.partial[(int64_t)blockIdx.y * a.n + t] = double2{ax, ay};
    return;
  }
  direct64_out(a, t, ax, ay);
}

// FAST with gsplit > 1: the splits' partial sums in split order, then the output.
__global__ __launch_bounds__(256) void direct64_finish(const Direct64Args a) {
  if (*a.domain_flag != 0) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n) return;
  double2 s = a.partial[t];
  for (int g = 1; g < a.gsplit; ++g) {
    const double2 r = a.partial[(int64_t)g * a.n + t];
    s.x = s.x + r.x;
    s.y = s.y + r.y;
  }
  direct64_out(a, t, s.x, s.y);
}

// The FAST domain of direct64.h (fast_domain.h), every coordinate: finite, below 2^100 in magnitude, zero or at least 2^-300.
__global__ __launch_bounds__(256) void direct64_domain_scan(const double* xy, int64_t n_doubles, int* flag) {
  bool out = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_doubles; i += (int64_t)gridDim.x * 256) {
    const double v = __builtin_fabs(xy[i]);
    out |= !(v < kFastBig64) || (v != 0.0 && v < kFastTiny64);  // outside_fast (fast_domain.h), spelled out: (a NaN fails the first test)
  }
  if (__builtin_amdgcn_ballot_w64(out) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// Sources split over blockIdx.y for FAST until there are ~16 waves per SIMD (256 CUs x 4 SIMDs), a split >= 2048 sources.
int direct64_gsplit(int64_t n) {
  const int64_t waves = (n + 63) / 64;
  int64_t g = waves > 0 ? (16384 + waves - 1) / waves : 1;
  if (g > 16) g = 16;
  while (g > 1 && n / g < 2048) g /= 2;
  return g < 1 ? 1 : (int)g;
}

template <bool FAST, int TB> void launch_pass(hipStream_t s, const Direct64Args& a, int gsplit) {
  hipLaunchKernelGGL((direct64_pass<FAST, TB>), dim3((unsigned)((a.n + 255) / 256), (unsigned)gsplit), dim3(256), 0, s, a);
}

}  // namespace

size_t direct64_ws_bytes(int64_t n) {
  const int g = direct64_gsplit(n);
  return kFlag64Bytes + (g > 1 ? (size_t)g * (size_t)n * sizeof(double2) : 0);
}

hipError_t launch_direct64(hipStream_t s, Direct64Args a, bool fast, void* ws, size_t ws_bytes) {
  if (a.n <= 0) return hipSuccess;
  if (!ws || ws_bytes < kFlag64Bytes) return hipErrorInvalidValue;
  // Laboratory: NBODY_DIRECT64_TB the EXACT term block (4 / 8 / 16), NBODY_DIRECT64_GSPLIT FAST's source splits
  const int tb = lab_int("NBODY_DIRECT64_TB", 8);
  if (!fast) {
    a.domain_flag = nullptr;
    a.gsplit = 1;
#ifdef NBODY_LAB
    if (tb == 4) launch_pass<false, 4>(s, a, 1);
    else if (tb == 16) launch_pass<false, 16>(s, a, 1);
    else launch_pass<false, 8>(s, a, 1);
#else
    (void)tb;
    launch_pass<false, 8>(s, a, 1);
#endif
    return hipGetLastError();
  }
  int* flag = (int*)ws;
  a.domain_flag = flag;
  int g = lab_int("NBODY_DIRECT64_GSPLIT", direct64_gsplit(a.n));
  if (g < 1) g = 1;
  if (g > 64) g = 64;
  while (g > 1 && kFlag64Bytes + (size_t)g * (size_t)a.n * sizeof(double2) > ws_bytes) --g;  // (an override may not fit)
  a.gsplit = g;
  a.partial = g > 1 ? (double2*)((char*)ws + kFlag64Bytes) : nullptr;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  int64_t blocks = (2 * a.n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(direct64_domain_scan, dim3((unsigned)blocks), dim3(256), 0, s, (const double*)a.pos, 2 * a.n, flag);
  launch_pass<true, 8>(s, a, g);
  if (g > 1) hipLaunchKernelGGL(direct64_finish, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  launch_pass<false, 8>(s, a, 1);  // the fallback: returns at once when the scan found every position inside the domain
  return hipGetLastError();
}

}  // namespace nbody
