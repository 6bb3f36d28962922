// Frames of an ensemble (nbody_frames_*): every world's draw() raster (render.hip) from one call, for all eight ensemble handles.
// Internal.  A frame is [n_worlds][render_px][render_px] uchar4, world k's tile the draw() of its own rows alone: its bodies in
// upload order (ensemble rows never move) and then, where the caller asks for them, its tracers as rows n .. n+m-1 of weight 1.
//
// One kernel text over T (float / double) serves every handle.  What differs between the handles is in FrameArgs:
//   mass     the f32 handles keep `weight as f32`, the f64 handles the u32 weights; frame_heavy() below is one predicate on both;
//   rows     a uniform handle (n_bodies, n_tracers the same in every world) computes a world's row ranges from its index; a
//            ragged one reads them from `table`, one WorldRanges per world (ensemble_rows.h), which the driver builds from the
//            sizes it holds.
//
// Two routes, chosen by render_px alone (frame_route_lds):
//   LDS      render_px^2 * 8 <= 81 920 B (render_px <= 101; 81 920 B is the dynamic LDS the f64 ensemble already raises its
//            kernels to on this device).  One 256-thread block per world; the world's two words per pixel live in dynamic LDS:
//            zero, barrier, splat bodies then tracers with LDS atomics (results unused: the no-return forms), barrier, resolve
//            straight to the world's tile with coalesced stores.  No global atomics, no memset, one launch for all worlds.
//   global   above that: two u32 per pixel per world in `work` (zeroed by the call with hipMemsetAsync), one splat launch over
//            (world, 256-row chunk), one resolve launch over all pixels.
// Both routes produce the same bytes by construction: the three facts per pixel (render.hip) are order-free.  NO crossover
// between the routes has been measured: the rule is "what fits in LDS goes there".  profiles/ensemble_frames.txt holds whole
// calls of both routes at neighbouring render_px (100 and 125) as recorded figures, not as a threshold: per pixel of all worlds
// the two are within a tenth of each other there (the copy to the host and the launches included), so those figures do not
// show the LDS route to be the faster one at render_px = 100; nothing sends 100 down the global route, so that is unmeasured.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ensemble_rows.h"

namespace nbody {

constexpr size_t kFrameLdsBytes = 81920;            // = ensemble64_lds_bytes(kEnsembleMaxBodies): what ens64_raise_lds_limit raises a kernel to
constexpr int64_t kFrameMaxPixels = 1ll << 26;      // n_worlds * render_px^2
constexpr int64_t kFrameMaxRows = 1ll << 24;        // per world, bodies and tracers together: a row shares a word with its v
constexpr uint32_t kFrameMaxHeight = 1u << 24;      // `height as T` exact in f32, as nbody_render_rgba asks

inline bool frame_route_lds(uint32_t render_px) { return (size_t)render_px * render_px * 8 <= kFrameLdsBytes; }

struct FrameArgs {
  const void* pos = nullptr;    // T2 rows of all worlds (the handle's current buffer)
  const void* vel = nullptr;
  const void* mass = nullptr;   // float rows (T = float) or uint32_t rows (T = double)
  const void* tpos = nullptr;   // tracers, or NULL: bodies only
  const void* tvel = nullptr;
  const WorldRanges* table = nullptr;  // ragged: one per world (device); NULL: uniform
  uint32_t n_bodies = 0, n_tracers = 0;  // uniform: per world
  uint32_t chunks = 0;          // global route: 256-row chunks per world, of the largest world (set by the launch)
  uint32_t height = 0, render_px = 0;
};

// All worlds' frames on `s`.  max_rows: the largest n + m among the worlds (<= kFrameMaxRows).  work: 2 * n_worlds *
// render_px^2 u32 on the global route (zeroed by the call), unused (may be NULL) on the LDS route.  rgba: n_worlds *
// render_px^2 * 4 bytes of device memory.  Arguments outside the limits above come back as hipErrorInvalidValue, never as a launch.
template <class T>
hipError_t launch_ensemble_frames(hipStream_t s, int64_t n_worlds, int64_t max_rows, FrameArgs a, uint32_t* work, uint8_t* rgba);

}  // namespace nbody
