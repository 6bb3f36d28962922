"""Rates of the direct sum at arbitrary points (nbody_accel_direct_at_*, Context.accel_direct(targets)).

Each case is one call of the C ABI, timed by a synchronised host clock (the call returns once its results are on the host, so
the time includes the targets' upload and the results' download): the median of --reps calls after --warmup.  Printed per
case: ms per call, pairs/s, TFLOP/s at 14 flops per pair (as bench.py counts them) and the share of the f32 (157.3 TFLOP/s)
or f64 (78.6 TFLOP/s) vector peak.  One JSON line per case; needs an MI355X.

    python tools/probe_bench.py [--reps 5] [--warmup 2] [--only NAME ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TFLOPS = 157.3
PEAK_F64_TFLOPS = 78.6
FLOPS_PER_PAIR = 14

# name, dtype, bodies, targets, arith, masses
CASES = [
    ("f32_fast_1M_x_1M", np.float32, 1 << 20, 1 << 20, "fast", "equal"),
    ("f32_fast_1M_x_1M_free_masses", np.float32, 1 << 20, 1 << 20, "fast", "free"),
    ("f32_fast_4096_x_1M", np.float32, 1 << 20, 4096, "fast", "equal"),
    ("f32_exact_65536_x_65536", np.float32, 65536, 65536, "exact", "equal"),
    ("f64_exact_65536_x_65536", np.float64, 65536, 65536, "exact", "equal"),
    ("f64_fast_65536_x_65536", np.float64, 65536, 65536, "fast", "equal"),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    import nbody_simulation_amd as nb
    C = nb._capi
    arith_of = {"fast": C.ARITH_FAST, "exact": C.ARITH_EXACT, "auto": C.ARITH_AUTO}
    with C.Context(0) as ctx:
        for name, dt, n, m, arith, masses in CASES:
            if args.only and name not in args.only:
                continue
            pos, vel, w = nb.scenes.plummer(n, seed=0x9B0BE, dtype=dt)
            if masses == "free":
                w = np.random.default_rng(1).integers(1, 1 << 20, n).astype(np.uint32)
            rng = np.random.default_rng(2)
            tgt = (pos[rng.integers(0, n, m)] + rng.normal(0, 10, (m, 2))).astype(dt)
            ctx.set_params(arith=arith_of[arith])
            ctx.upload(pos, vel, w)
            for _ in range(args.warmup):
                ctx.accel_direct(tgt)
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                ctx.accel_direct(tgt)
                times.append(time.perf_counter() - t0)
            s = float(np.median(times))
            pairs = float(n) * float(m)
            tflops = FLOPS_PER_PAIR * pairs / s / 1e12
            peak = PEAK_F64_TFLOPS if dt == np.float64 else PEAK_F32_TFLOPS
            print(json.dumps({"case": name, "bodies": n, "targets": m, "arith": arith, "masses": masses,
                              "ms_median": round(1e3 * s, 3), "ms_min": round(1e3 * min(times), 3),
                              "ms_runs": [round(1e3 * t, 3) for t in times],
                              "pairs_per_s": float(f"{pairs / s:.4g}"), "tflops": round(tflops, 2),
                              "frac_of_peak": round(tflops / peak, 3), "peak_tflops": peak,
                              "timing": "host clock around the synchronous call (includes target upload, result download)"}),
                  flush=True)


if __name__ == "__main__":
    main()
