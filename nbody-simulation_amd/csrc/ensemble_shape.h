// Ensembles: the limits and the functions of a world's size that decide its launch — how many lanes share a target and
// how much LDS its sources take, in f32 and in f64.  Internal.  Plain C++ (no HIP include), so that the host-only plan of ragged_plan.h and a
// stand-alone host program can use them; the kernels see the same definitions through ensemble_kernels.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NB_ENS_HD __host__ __device__
#else
#define NB_ENS_HD
#endif

namespace nbody {

constexpr int kEnsembleMaxBodies = 4096;
constexpr int64_t kEnsembleMaxRows = 1ll << 26;  // the rows of all worlds together
constexpr int kEnsembleBlock = 256;

// Lanes that share one target's sources.
NB_ENS_HD inline int ensemble_split(int n_bodies) {
  if (n_bodies > 128) return 1;
  int split = 2, targets = 128;
  while (targets / 2 >= n_bodies && split < 64) { targets /= 2; split *= 2; }
  return split;
}
inline size_t ensemble_lds_bytes(int n_bodies) { return (size_t)((n_bodies + 1) / 2) * 24; }  // couples {xA, xB, yA, yB} + {mA, mB}

// In f64 (ensemble64_kernels.h): rows padded to a multiple of the EXACT term block, a double2 position and a u32 weight each.
constexpr int kEns64TermBlock = 8;  // EXACT: pairs evaluated together before their terms are added in ascending j
inline int ensemble64_padded(int n_bodies) { return (n_bodies + kEns64TermBlock - 1) / kEns64TermBlock * kEns64TermBlock; }
inline size_t ensemble64_lds_bytes(int n_bodies) { return (size_t)ensemble64_padded(n_bodies) * (2 * sizeof(double) + sizeof(uint32_t)); }

}  // namespace nbody
