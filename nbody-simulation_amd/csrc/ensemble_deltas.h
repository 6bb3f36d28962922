// Delta streams of an ensemble (nbody_deltas_*): one NBD1 stream (delta_codec.h) per world from one call, for all eight
// ensemble handles.  Internal.  A *segment* is one world's bodies or one world's tracers: n rows in upload order (ensemble
// rows never move, so there are no ids and no scatter).  Every segment's stream is byte for byte what the single-sequence
// encoder (delta_snapshot.hip) gives for a context holding that segment alone; the per-block arithmetic is shared with it
// (delta_device.h).
//
// One kernel text over the key type K (uint32_t / uint64_t) serves every handle and both sequences (bodies, tracers).
// What differs between the handles is in DeltasArgs:
//   uniform   n rows in every segment: a block's segment is its index divided by the blocks per segment;
//   ragged    `table`, one DeltaSeg per segment, and `seg_of_block`, one entry per 64-row block, built on the host once
//             per upload.
// A call is a fixed number of launches, whatever the number of worlds:
//   widths    one wave = one 64-row block of one segment: the rows straight from the positions (zero keys for lanes past
//             n), the keys stored as `cur`, both coordinates' width bytes and word counts;
//   scan      one exclusive sum over the 2 * blocks + 1 word counts (the last entry is the total);
//   pack      the residuals recomputed, every bit plane one ballot, the payload words and the block's two width bytes
//             written at their final place in the output;
//   headers   one thread per segment: the 32-byte header, the padding of the width bytes, the stream's offset.
// Stream k starts at base_k + 8 * (words before segment k), base_k = sum_{j<k} (32 + width_bytes(n_j)): known at upload.
// Word offsets are 32-bit: at most 2^24 blocks per call (2 * 2^24 * 64 = 2^31 words), which the driver refuses above.
// The passes are memory bound: per row one 8 B / 16 B load, three key loads and one key store per coordinate in `widths`,
// three key loads per coordinate in `pack`, and 8-byte payload stores.  Nothing of this has a measured alternative.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "delta_codec.h"

namespace nbody {

constexpr int64_t kDeltasMaxBlocks = 1ll << 24;  // 64-row blocks of all addressed segments together

struct DeltaSeg {      // a ragged segment (24 bytes)
  uint32_t row0, n;    // rows [row0, row0 + n) of the positions
  uint32_t blk0, pad;  // its first 64-row block among the blocks of all segments
  uint64_t base;       // sum over the segments before it of (32 + width bytes)
};

struct DeltasArgs {
  const void* pos = nullptr;               // K pairs: the rows of all segments (bodies: the current buffer; or the tracers)
  const DeltaSeg* table = nullptr;         // ragged: one per segment (device); NULL: uniform
  const uint32_t* seg_of_block = nullptr;  // ragged: one per block (device)
  uint32_t n_segs = 0, n = 0;              // n: uniform rows per segment
  uint32_t blocks = 0;                     // of all segments, <= 2^24
  uint32_t have = 0;                       // how many of prev, prev2 hold keys (0: key frame; 1: prev2 reads as zero)
  uint64_t step = 0;
  uint64_t base_total = 0;                 // sum over all segments of (32 + width bytes)
  void* cur = nullptr;                     // keys, [2 * block + coordinate][64]
  const void* prev = nullptr;
  const void* prev2 = nullptr;
  uint8_t* widths = nullptr;               // [2 * block + coordinate]
  uint32_t* words = nullptr;               // [2 * blocks + 1]
  uint32_t* offsets = nullptr;             // [2 * blocks + 1], the exclusive sum of words
  uint8_t* out = nullptr;                  // the streams, one after another
  uint64_t* stream_off = nullptr;          // [n_segs + 1]: every stream's offset in out, then the total
};

size_t deltas_scan_temp_bytes(int64_t blocks);

// widths and the scan, on `s`: afterwards a.offsets[2 * blocks] is the payload of all segments in words.  blocks >= 1.
template <class K> hipError_t launch_deltas_measure(hipStream_t s, const DeltasArgs& a, void* scan_temp, size_t scan_temp_bytes);
// pack (where blocks >= 1) and headers, on `s`: a.out holds every stream, a.stream_off their offsets.
template <class K> hipError_t launch_deltas_write(hipStream_t s, const DeltasArgs& a);

}  // namespace nbody
