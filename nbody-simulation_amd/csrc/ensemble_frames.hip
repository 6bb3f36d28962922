// Frames of an ensemble: the reference's draw() (src/main.rs:41-72) of every world's own rows, all worlds from one call
// (ensemble_frames.h).  The per-pixel semantics are render.hip's, stated at its top, per world:
//   a row inside [0, height)^2 touches the pixel (y as u32 / cell) * render_px + (x as u32 / cell), cell = height / render_px;
//   a heavy row (weight > 10) sets the pixel's heavy bit;
//   a light row adds 1 to the pixel's count and takes an atomic max of (row << 8) | v, v = 0x10 + min(((|vx|+|vy|)*10) as u8, 0xef):
//     the LAST light row in row order colours the pixel, whatever its v;
//   resolve: heavy -> (0,255,0,255); no row -> 0; else (255, 255-v, 255-v, min(10*count, 250)).
// `row` is the row's index within its world: bodies 0 .. n-1 in upload order, then the tracers n .. n+m-1, every tracer light.
// The float-to-integer casts and their NaN / saturation behaviour are render_splat's, line for line.
//
// The two routes (LDS: one block per world, the words in dynamic LDS; global: the words in a work buffer) share frame_splat_row
// and frame_pixel, so their bytes cannot differ: only where the two words per pixel live does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble64_kernels.h"
#include "ensemble_frames.h"

namespace nbody {

namespace {

template <class T> struct FrameTypes;
template <> struct FrameTypes<float> { using Vec2 = float2; using Mass = float; };
template <> struct FrameTypes<double> { using Vec2 = double2; using Mass = uint32_t; };

constexpr uint32_t kFrameHeavyBit = 0x80000000u;
constexpr int kFrameBlock = 256;

// draw()'s `weight > 10`.  The f64 handles keep the u32 weights.  The f32 handles keep mass = weight as f32: u32 -> f32 is
// monotone (round to nearest never reorders) and 10 and 11 are exact, so weight <= 10 gives mass <= 10.0f and weight >= 11 gives
// mass >= 11.0f: `mass > 10.0f` is the same predicate, and the f32 handles need no weight array.
__device__ __forceinline__ bool frame_heavy(uint32_t weight) { return weight > 10u; }
__device__ __forceinline__ bool frame_heavy(float mass) { return mass > 10.0f; }

// A world's rows: from the table (ragged) or from its index (uniform).  The same in every lane of a block.
__device__ __forceinline__ WorldRanges frame_world(const FrameArgs& a, uint32_t world) {
  if (a.table) {
    const uint4 w = reinterpret_cast<const uint4*>(a.table)[world];
    return WorldRanges{w.x, w.y, w.z, a.tpos ? w.w : 0u};  // (the table keeps the counts; the call says whether they are painted)
  }
  return WorldRanges{world * a.n_bodies, a.n_bodies, world * a.n_tracers, a.tpos ? a.n_tracers : 0u};  // (rows of all worlds <= 2^26)
}

// Row r of the world (r < w.n + w.m) splatted into the world's words.  The atomics' results are unused.
template <class T>
__device__ __forceinline__ void frame_splat_row(const FrameArgs& a, const WorldRanges& w, uint32_t r, T height, uint32_t cell,
                                                uint32_t* count, uint32_t* last) {
  using T2 = typename FrameTypes<T>::Vec2;
  using Mass = typename FrameTypes<T>::Mass;
  const bool body = r < w.n;
  const size_t i = body ? (size_t)w.row0 + r : (size_t)w.trow0 + (r - w.n);
  const T2 p = reinterpret_cast<const T2*>(body ? a.pos : a.tpos)[i];
  if (!(p.y < height && p.x < height && p.y >= (T)0 && p.x >= (T)0)) return;  // within_bounds; NaN fails
  const uint32_t px = (uint32_t)p.x / cell, py = (uint32_t)p.y / cell;        // `as u32` truncates
  const uint32_t pix = py * a.render_px + px;
  if (body && frame_heavy(reinterpret_cast<const Mass*>(a.mass)[i])) {
    atomicOr(&count[pix], kFrameHeavyBit);
    return;
  }
  const T2 v = reinterpret_cast<const T2*>(body ? a.vel : a.tvel)[i];
  const T t = ((v.x < 0 ? -v.x : v.x) + (v.y < 0 ? -v.y : v.y)) * (T)10.0;
  uint32_t b = t != t ? 0u : (t >= (T)255 ? 255u : (uint32_t)t);  // `as u8` saturates, NaN -> 0
  b = b < 0xefu ? b : 0xefu;
  atomicAdd(&count[pix], 1u);
  atomicMax(&last[pix], (r << 8) | (0x10u + b));  // rows < 2^24
}

__device__ __forceinline__ uchar4 frame_pixel(uint32_t c, uint32_t l) {
  if (c & kFrameHeavyBit) return make_uchar4(0x00, 0xff, 0x00, 0xff);
  if (!c) return make_uchar4(0, 0, 0, 0);
  const uint32_t v = l & 0xffu;
  const uint32_t al = c < 25u ? 10u * c : 250u;
  return make_uchar4(0xff, (unsigned char)(0xffu - v), (unsigned char)(0xffu - v), (unsigned char)al);
}

// ---- LDS route: block = world.  Dynamic LDS: count[npix] then last[npix].
template <class T>
__global__ __launch_bounds__(kFrameBlock) void ensemble_frames_lds(const FrameArgs a, uchar4* __restrict__ rgba) {
  extern __shared__ __attribute__((aligned(16))) uint32_t frame_lds[];
  const uint32_t npix = a.render_px * a.render_px, cell = a.height / a.render_px;
  uint32_t* const count = frame_lds;
  uint32_t* const last = frame_lds + npix;
  const WorldRanges w = frame_world(a, blockIdx.x);
  for (uint32_t i = threadIdx.x; i < 2 * npix; i += kFrameBlock) frame_lds[i] = 0u;
  __syncthreads();
  const uint32_t rows = w.n + w.m;  // bodies first, then tracers: one loop, the rows in order of their index
  for (uint32_t r = threadIdx.x; r < rows; r += kFrameBlock) frame_splat_row<T>(a, w, r, (T)a.height, cell, count, last);
  __syncthreads();
  uchar4* const tile = rgba + (size_t)blockIdx.x * npix;
  for (uint32_t i = threadIdx.x; i < npix; i += kFrameBlock) tile[i] = frame_pixel(count[i], last[i]);
}

// ---- global route: block = (world, 256-row chunk), the words of world k at work[2 k npix ..): count then last.
template <class T>
__global__ __launch_bounds__(kFrameBlock) void ensemble_frames_splat(const FrameArgs a, uint32_t* __restrict__ work) {
  const uint32_t npix = a.render_px * a.render_px, cell = a.height / a.render_px;
  const uint32_t world = blockIdx.x / a.chunks, chunk = blockIdx.x - world * a.chunks;
  const WorldRanges w = frame_world(a, world);
  const uint32_t r = chunk * kFrameBlock + threadIdx.x;
  if (r >= w.n + w.m) return;
  uint32_t* const count = work + (size_t)world * 2 * npix;
  frame_splat_row<T>(a, w, r, (T)a.height, cell, count, count + npix);
}

__global__ __launch_bounds__(kFrameBlock) void ensemble_frames_resolve(uint32_t total, uint32_t npix, const uint32_t* __restrict__ work,
                                                                       uchar4* __restrict__ rgba) {
  const uint32_t i = blockIdx.x * kFrameBlock + threadIdx.x;  // total <= 2^26
  if (i >= total) return;
  const uint32_t world = i / npix, pix = i - world * npix;
  const uint32_t* const count = work + (size_t)world * 2 * npix;
  rgba[i] = frame_pixel(count[pix], count[npix + pix]);
}

}  // namespace

template <class T>
hipError_t launch_ensemble_frames(hipStream_t s, int64_t n_worlds, int64_t max_rows, FrameArgs a, uint32_t* work, uint8_t* rgba) {
  const int64_t npix = (int64_t)a.render_px * a.render_px;
  if (n_worlds < 1 || a.render_px == 0 || a.height == 0 || a.height > kFrameMaxHeight || a.height % a.render_px != 0 ||
      n_worlds > kFrameMaxPixels / npix || max_rows < 1 || max_rows > kFrameMaxRows || !rgba || !a.pos || !a.vel || !a.mass ||
      (a.tpos && !a.tvel))
    return hipErrorInvalidValue;
  if (frame_route_lds(a.render_px)) {
    const size_t lds = (size_t)npix * 8;
    if (lds > 65536) {  // above 64 KB the function's limit is raised, once per device (to kFrameLdsBytes exactly)
      static std::atomic<bool> raised[64];
      const hipError_t h = ens64_raise_lds_limit(reinterpret_cast<const void*>(&ensemble_frames_lds<T>), raised);
      if (h != hipSuccess) return h;
    }
    hipLaunchKernelGGL(ensemble_frames_lds<T>, dim3((unsigned)n_worlds), dim3(kFrameBlock), lds, s, a, (uchar4*)rgba);
    return hipGetLastError();
  }
  // render_px >= 102 here, so n_worlds <= 2^26 / 10404 = 6450 and, with at most 2^16 chunks, the grid stays below 2^29 blocks
  if (!work) return hipErrorInvalidValue;
  a.chunks = (uint32_t)((max_rows + kFrameBlock - 1) / kFrameBlock);
  const int64_t total = n_worlds * npix;
  hipError_t h = hipMemsetAsync(work, 0, sizeof(uint32_t) * 2 * (size_t)total, s);
  if (h != hipSuccess) return h;
  hipLaunchKernelGGL(ensemble_frames_splat<T>, dim3((unsigned)(n_worlds * a.chunks)), dim3(kFrameBlock), 0, s, a, work);
  hipLaunchKernelGGL(ensemble_frames_resolve, dim3((unsigned)((total + kFrameBlock - 1) / kFrameBlock)), dim3(kFrameBlock), 0, s,
                     (uint32_t)total, (uint32_t)npix, work, (uchar4*)rgba);
  return hipGetLastError();
}

template hipError_t launch_ensemble_frames<float>(hipStream_t, int64_t, int64_t, FrameArgs, uint32_t*, uint8_t*);
template hipError_t launch_ensemble_frames<double>(hipStream_t, int64_t, int64_t, FrameArgs, uint32_t*, uint8_t*);

}  // namespace nbody
