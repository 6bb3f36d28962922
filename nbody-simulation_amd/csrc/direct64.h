// Launch interface of the f64 direct O(N^2) step (direct64.hip).  Internal to the library.
//
// EXACT (the default, and what AUTO runs): per target one chain of IEEE additions in double, ascending source index, each
// term the reference's pair in T = double (pair_term_select, the branch-free pair_term_t<double>, pair.h); integration fused
// (main.rs:419-423, no contraction).
// Bit-identical to the oracle's orc_direct_accel_f64 / orc_update_direct_f64.
//
// FAST (opt-in): the f64 walk's FAST pair (2^-700-biased denominator, v_rcp_f64 + one Newton step, FMAs), the sources split
// over blockIdx.y and the partial sums added in fixed order by a finish kernel (bitwise reproducible).  Contract:
// |a - a_ref|_1 <= 1e-12 * sum_j |term_ij|_1 per body.  It holds inside the FAST domain, which a device-side scan checks every
// step; a step with any position outside it runs the EXACT kernel instead (no host round trip):
//   every coordinate finite, and |v| < 2^100, and v == 0 or |v| >= 2^-300; and the clamp > 0 (checked on the host).
// Inside it no difference, square or denominator overflows (den < 2^305), a non-zero separation is >= 2^-352 so the bias is
// below 2^-199 of any denominator, and a coincident pair contributes exactly 0.
//
// Not provided for f64: multi-device or sharded direct steps (the *_dev entry points), mass classes, the near/far split,
// and graph replay of small steps.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nbody {

struct Direct64Args {
  const double2* pos = nullptr;   // [n] sources = targets
  const double* mass = nullptr;   // [n] `weight as f64`
  int64_t n = 0;
  double2* vel = nullptr;         // with pos_out: integrate (vel in place)
  double2* pos_out = nullptr;
  double2* acc_out = nullptr;     // optional: the accelerations
  double2* partial = nullptr;     // FAST with gsplit > 1: [gsplit][n]
  double delta = 0, clamp = 0;
  int gsplit = 1;
  const int* domain_flag = nullptr;  // FAST step: != 0 when a position is outside the FAST domain
};

// The workspace of an f64 direct step of n bodies: the domain flag and the FAST partial sums.
size_t direct64_ws_bytes(int64_t n);
// One step.  fast: scan + FAST kernels + the EXACT kernel gated on the scan's verdict; otherwise the EXACT kernel only.
hipError_t launch_direct64(hipStream_t s, Direct64Args a, bool fast, void* ws, size_t ws_bytes);

}  // namespace nbody
