// Internal: where the parts of a direct step's workspace lie.  direct_layout() (direct_driver.hip) is the only place that places
// them; everything else reads a DirectLayout through the accessors below.
#pragma once
#include "direct_kernels.h"

namespace nbody {

struct DirectLayout {
  static constexpr size_t kNoMutual = ~(size_t)0;
  static constexpr size_t flags = 0;  // the decision words (kFlagHazard ...) open every workspace, whatever its sizes
  size_t partial = 0, partial_bytes = 0;  // [gsplit][n_tgt] partial sums of one run
  size_t nearfar = 0;                     // the near/far scratch, laid out by `nf`
  NearFarLayout nf{};
  size_t mutual = kNoMutual;              // the mutual pass's strip buffers; kNoMutual where the pass cannot engage
  size_t total = 0;
};
// n_tgt_max: the largest block of targets one run covers
DirectLayout direct_layout(int64_t n_src, int64_t n_tgt_max);

inline int* direct_flags(void* ws) { return (int*)((char*)ws + DirectLayout::flags); }
inline float2* direct_partial(void* ws, const DirectLayout& L) { return (float2*)((char*)ws + L.partial); }
inline char* direct_nearfar(void* ws, const DirectLayout& L) { return (char*)ws + L.nearfar; }
inline const float2* direct_pos_far(void* ws, const DirectLayout& L) { return (const float2*)(direct_nearfar(ws, L) + L.nf.pos_far); }
inline const uint32_t* direct_near_list(void* ws, const DirectLayout& L) { return (const uint32_t*)(direct_nearfar(ws, L) + L.nf.near_list); }
inline const float* direct_minv_far(void* ws, const DirectLayout& L) { return (const float*)(direct_nearfar(ws, L) + L.nf.minv_far); }
inline MutualArea direct_mutual_area(void* ws, const DirectLayout& L, int64_t n_src) {
  const char* nf = direct_nearfar(ws, L);
  return mutual_area((char*)ws + L.mutual, n_src, (const uint32_t*)(nf + L.nf.is_near), (const uint32_t*)(nf + L.nf.scan));
}

}  // namespace nbody
