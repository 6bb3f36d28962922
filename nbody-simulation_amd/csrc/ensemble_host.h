// What the two ensemble drivers (ensemble.hip, ensemble64.hip) share on the host: the device probe and the stream of a handle.
// Internal.  Everything typed — arrays, arguments, the kernel — stays in the driver of its precision.
#pragma once
#include <cstring>
#include <string>

#include "driver.h"

namespace nbody {

// Checks that device_id is a gfx950, makes it current and creates the handle's stream.  `who` is the create call's name, the
// prefix of every message.  -> NBODY_OK, or the error code with `msg` set (and no stream).
inline int ensemble_open_device(const char* who, int device_id, hipStream_t* stream, std::string& msg) {
  *stream = nullptr;
  int count = 0;
  hipError_t h = hipGetDeviceCount(&count);
  if (h != hipSuccess || count <= 0) {
    msg = std::string(who) + ": no HIP device (" + (h != hipSuccess ? hipGetErrorString(h) : "count 0") + "); this library has no CPU path";
    return NBODY_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= count) {
    msg = std::string(who) + ": device_id out of range";
    return NBODY_ERR_INVALID;
  }
  hipDeviceProp_t prop;
  h = hipGetDeviceProperties(&prop, device_id);
  if (h != hipSuccess) {
    msg = std::string("ensemble: hipGetDeviceProperties: ") + hipGetErrorString(h);
    return NBODY_ERR_HIP;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    msg = std::string(who) + ": device is " + prop.gcnArchName + ", kernels are built for gfx950 (MI355X) only";
    return NBODY_ERR_NO_DEVICE;
  }
  h = hipSetDevice(device_id);
  if (h == hipSuccess) h = hipStreamCreateWithFlags(stream, hipStreamNonBlocking);
  if (h != hipSuccess) {
    *stream = nullptr;
    msg = std::string("ensemble: ") + who + ": " + hipGetErrorString(h);
    return NBODY_ERR_HIP;
  }
  return NBODY_OK;
}

// Before a handle's buffers are freed: its device current, its stream drained.  After: ensemble_close_stream.
inline void ensemble_drain(int device, hipStream_t stream) {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
}
inline void ensemble_close_stream(hipStream_t stream) {
  if (stream) (void)hipStreamDestroy(stream);
}

}  // namespace nbody
