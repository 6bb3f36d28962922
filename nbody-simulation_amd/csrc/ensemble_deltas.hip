// Delta streams of an ensemble: the batched NBD1 encoder of ensemble_deltas.h, and nbody_deltas_bound.  One wave is one
// 64-row block of one segment, so a bit plane of a block is exactly one ballot, as in delta_snapshot.hip, whose per-block
// arithmetic this file shares through delta_device.h.
#include "ensemble_deltas.h"

#include <hipcub/hipcub.hpp>

#include "delta_device.h"
#include "driver.h"

namespace nbody {
namespace {

// A row's two coordinates as bit patterns: one 8-byte (f32) or 16-byte (f64) load.
template <class K> struct alignas(2 * sizeof(K)) KeyPair { K x, y; };

__device__ __forceinline__ uint32_t deltas_width_bytes(uint32_t n) { return (2 * ((n + 63) / 64) + 7) / 8 * 8; }

// A segment's rows and place: from the table (ragged) or from its index (uniform).
__device__ __forceinline__ DeltaSeg deltas_segment(const DeltasArgs& a, uint32_t seg) {
  if (a.table) return a.table[seg];
  const uint32_t bps = (a.n + 63) / 64;  // (rows of all segments <= 2^26, blocks <= 2^24)
  return DeltaSeg{seg * a.n, a.n, seg * bps, 0u, (uint64_t)seg * (kDeltaHeader + deltas_width_bytes(a.n))};
}
// The segment of a block (blk < a.blocks, so a uniform segment has at least one block).  The same in every lane of a wave.
__device__ __forceinline__ uint32_t deltas_seg_of_block(const DeltasArgs& a, uint32_t blk) {
  return a.table ? a.seg_of_block[blk] : blk / ((a.n + 63) / 64);
}

template <class K> __device__ __forceinline__ void deltas_history(const DeltasArgs& a, size_t at, K& p1, K& p2) {
  p1 = a.have >= 1 ? reinterpret_cast<const K*>(a.prev)[at] : (K)0;
  p2 = a.have >= 2 ? reinterpret_cast<const K*>(a.prev2)[at] : (K)0;
}

// One wave per block, both coordinates: the keys of the rows, the width byte and the payload words of each (block, coordinate).
template <class K> __global__ __launch_bounds__(256) void deltas_widths(const DeltasArgs a) {
  const uint32_t blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= a.blocks) return;
  const uint32_t lane = threadIdx.x & 63;
  const DeltaSeg s = deltas_segment(a, deltas_seg_of_block(a, blk));
  const uint32_t r = (blk - s.blk0) * 64 + lane;
  K key[2] = {0, 0};  // lanes past n: zero keys, hence z = 0
  if (r < s.n) {
    const KeyPair<K> p = reinterpret_cast<const KeyPair<K>*>(a.pos)[(size_t)s.row0 + r];
    key[0] = delta_key(p.x);
    key[1] = delta_key(p.y);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const size_t at = ((size_t)2 * blk + c) * 64 + lane;
    reinterpret_cast<K*>(a.cur)[at] = key[c];
    K p1, p2, z0, z1;
    deltas_history<K>(a, at, p1, p2);
    residuals(key[c], p1, p2, z0, z1);
    const int w0 = bits_of(wave_or(z0)), w1 = bits_of(wave_or(z1));
    const int pred = w1 < w0 ? 1 : 0;
    const int w = pred ? w1 : w0;
    if (lane == 0) {
      a.widths[(size_t)2 * blk + c] = (uint8_t)(w | (pred << 7));
      a.words[(size_t)2 * blk + c] = (uint32_t)w;
    }
  }
}

template <class K> __global__ __launch_bounds__(256) void deltas_pack(const DeltasArgs a) {
  const uint32_t blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= a.blocks) return;
  const uint32_t lane = threadIdx.x & 63;
  const DeltaSeg s = deltas_segment(a, deltas_seg_of_block(a, blk));
  const uint32_t first = a.offsets[(size_t)2 * s.blk0];  // the words before this segment
  uint8_t* const stream = a.out + s.base + (size_t)first * 8;
  unsigned long long* const payload = reinterpret_cast<unsigned long long*>(stream + kDeltaHeader + deltas_width_bytes(s.n));
  uint32_t wbytes = 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const size_t at = ((size_t)2 * blk + c) * 64 + lane;
    const uint32_t wb = a.widths[(size_t)2 * blk + c];
    const uint32_t w = wb & 127u;
    wbytes |= wb << (8 * c);
    K p1, p2, z0, z1;
    deltas_history<K>(a, at, p1, p2);
    residuals(reinterpret_cast<const K*>(a.cur)[at], p1, p2, z0, z1);
    const K z = (wb & 128u) ? z1 : z0;
    unsigned long long mine = 0;
    for (uint32_t b = 0; b < w; ++b) {  // w is wave-uniform
      const unsigned long long plane = __ballot((z >> b) & 1);
      if (lane == b) mine = plane;
    }
    if (lane < w) payload[(size_t)(a.offsets[(size_t)2 * blk + c] - first) + lane] = mine;
  }
  if (lane == 0) *reinterpret_cast<uint16_t*>(stream + kDeltaHeader + 2 * (size_t)(blk - s.blk0)) = (uint16_t)wbytes;
}

// One thread per segment: header, the zero padding of the width bytes, the stream's offset (an empty segment is its header alone).
__global__ __launch_bounds__(256) void deltas_headers(const DeltasArgs a, uint32_t elem_bits) {
  const uint32_t seg = blockIdx.x * 256 + threadIdx.x;
  if (seg >= a.n_segs) return;
  const DeltaSeg s = deltas_segment(a, seg);
  const uint32_t nblk = (s.n + 63) / 64;
  const uint32_t first = a.offsets[(size_t)2 * s.blk0], end = a.offsets[(size_t)2 * (s.blk0 + nblk)];
  const uint64_t off = s.base + (uint64_t)first * 8;
  unsigned long long* const h = reinterpret_cast<unsigned long long*>(a.out + off);
  // 'N' 'B' 'D' '1', element bits, key frame, u16 0 (little endian)
  h[0] = 0x3144424eull | ((unsigned long long)elem_bits << 32) | ((unsigned long long)(a.have == 0 ? 1 : 0) << 40);
  h[1] = s.n;
  h[2] = a.step;
  h[3] = end - first;
  uint16_t* const pad = reinterpret_cast<uint16_t*>(a.out + off + kDeltaHeader);
  for (uint32_t i = nblk; i < deltas_width_bytes(s.n) / 2; ++i) pad[i] = 0;
  a.stream_off[seg] = off;
  if (seg == a.n_segs - 1) a.stream_off[a.n_segs] = a.base_total + (uint64_t)a.offsets[(size_t)2 * a.blocks] * 8;
}

bool deltas_args_ok(const DeltasArgs& a) {
  return a.n_segs >= 1 && (int64_t)a.blocks <= kDeltasMaxBlocks && a.have <= 2 && a.offsets && (!a.table || a.seg_of_block || !a.blocks);
}

}  // namespace

size_t deltas_scan_temp_bytes(int64_t blocks) {
  size_t tb = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(2 * blocks + 1), (hipStream_t) nullptr);
  return (tb + 255) / 256 * 256;
}

template <class K> hipError_t launch_deltas_measure(hipStream_t s, const DeltasArgs& a, void* scan_temp, size_t scan_temp_bytes) {
  if (!deltas_args_ok(a) || a.blocks < 1 || !a.pos || !a.cur || !a.prev || !a.prev2 || !a.widths || !a.words || !scan_temp)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((deltas_widths<K>), dim3((a.blocks + 3) / 4), dim3(256), 0, s, a);
  return hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_temp_bytes, (const uint32_t*)a.words, a.offsets, (int)(2 * a.blocks + 1), s);
}

template <class K> hipError_t launch_deltas_write(hipStream_t s, const DeltasArgs& a) {
  if (!deltas_args_ok(a) || !a.out || !a.stream_off || (a.blocks && (!a.cur || !a.prev || !a.prev2 || !a.widths))) return hipErrorInvalidValue;
  if (a.blocks) hipLaunchKernelGGL((deltas_pack<K>), dim3((a.blocks + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(deltas_headers, dim3((a.n_segs + 255) / 256), dim3(256), 0, s, a, (uint32_t)sizeof(K) * 8);
  return hipGetLastError();
}

template hipError_t launch_deltas_measure<uint32_t>(hipStream_t, const DeltasArgs&, void*, size_t);
template hipError_t launch_deltas_measure<uint64_t>(hipStream_t, const DeltasArgs&, void*, size_t);
template hipError_t launch_deltas_write<uint32_t>(hipStream_t, const DeltasArgs&);
template hipError_t launch_deltas_write<uint64_t>(hipStream_t, const DeltasArgs&);

}  // namespace nbody

using namespace nbody;

NB_API size_t nbody_deltas_bound(int64_t n_segments, const int64_t* rows, int is_f64) {
  if (n_segments < 0 || !rows) return 0;
  size_t bound = 0;
  int64_t blocks = 0;
  for (int64_t k = 0; k < n_segments; ++k) {
    if (rows[k] < 0 || rows[k] > kDeltasMaxBlocks * 64) return 0;
    blocks += (int64_t)delta_blocks(rows[k]);
    if (blocks > kDeltasMaxBlocks) return 0;
    bound += delta_bound(rows[k], is_f64 ? 64 : 32);
  }
  return bound;
}
